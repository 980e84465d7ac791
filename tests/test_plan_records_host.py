"""The plan-record expectation (tests/planref.py) and its comparer, without a GPU: the comparer must report every single
field it is given wrong, and the recipes of tests/test_gpu_plan_records.py must produce the material they promise, by the
oracle's records alone."""
from dataclasses import replace

import numpy as np
import pytest

import planrecipes
import planref

BLOCK = planref.BLOCK


@pytest.fixture(scope="module")
def sample(pkg, oracle):
    """Three blocks (probed, probed, a final block of 3000 frames compared in full) and their expectation as device output."""
    left, right = planrecipes.noise(2 * BLOCK + 3000, 16, 3)
    left[:256] = pkg.synth.synth_pcm(256, 1, 16, 48000, seed=9, kind="noise")[0]  # an LPC plan: coefficients to break
    exp = planref.expected_stream(oracle, left, right, 2)
    assert [sorted(b.slots) for b in exp][2] == [0, 1, 2, 3] and all(b.uncertain for b in exp)
    assert exp[0].slots[4].predictor_type == 2 and exp[0].slots[4].order >= 4
    assert any(len(r.part_mode_k) > 1 for r in exp[0].slots.values())
    return exp


def _returned(pkg, exp):
    return planref.to_ctypes(pkg.lacx, exp)


def test_comparer_accepts_the_expectation_itself(pkg, sample):
    bplans, plans = _returned(pkg, sample)
    assert planref.compare(sample, bplans, plans) == []
    planref.assert_same(sample, bplans, plans)
    full, probe = planref.counts(sample)
    assert (full, probe) == (2 + 2 + 4, 24)


SLOT_MUTATIONS = {
    "total_bits": lambda r: replace(r, total_bits=r.total_bits + 1),
    "payload_bytes": lambda r: replace(r, payload_bytes=r.payload_bytes + 1),
    "predictor_type": lambda r: replace(r, predictor_type=r.predictor_type ^ 2),
    "order": lambda r: replace(r, order=r.order + 1),
    "partition_order": lambda r: replace(r, partition_order=r.partition_order + 1),
    "coef[0]": lambda r: replace(r, coef=(r.coef[0] + 1,) + r.coef[1:]),
    "coef[last]": lambda r: replace(r, coef=r.coef[:-1] + (r.coef[-1] - 1,)),
    "part_mode_k[0] k": lambda r: replace(r, part_mode_k=(r.part_mode_k[0] ^ 1,) + r.part_mode_k[1:]),
    "part_mode_k[last] mode": lambda r: replace(r, part_mode_k=r.part_mode_k[:-1] + (r.part_mode_k[-1] ^ 0x20,)),
}


@pytest.mark.parametrize("what", sorted(SLOT_MUTATIONS))
def test_comparer_reports_one_wrong_slot_field(pkg, sample, what):
    """The device's answer differs from the oracle in exactly one field of one probe slot: exactly that is reported, with
    block, slot, window start, field and both values."""
    block, slot = 0, 4
    if what.startswith("part_mode_k"):
        slot = next(s for s, r in sample[0].slots.items() if len(r.part_mode_k) > 1)
    wrong = list(sample)
    slots = dict(wrong[block].slots)
    slots[slot] = SLOT_MUTATIONS[what](slots[slot])
    wrong[block] = replace(wrong[block], slots=slots)
    bplans, plans = _returned(pkg, wrong)
    diffs = planref.compare(sample, bplans, plans, stream="unit")
    field = what.split(" ")[0].replace("coef[last]", f"coef[{len(sample[0].slots[slot].coef) - 1}]") \
        .replace("part_mode_k[last]", f"part_mode_k[{len(sample[0].slots[slot].part_mode_k) - 1}]")
    assert len(diffs) == 1, diffs
    a, _ = planref.slot_window(BLOCK, slot)
    assert diffs[0].startswith(f"unit block 0 ({BLOCK} frames) slot {slot} ({'LRMS'[slot & 3]}, probe window {(slot >> 2) - 1} "
                               f"at frame {a}): {field} = "), diffs
    assert ", oracle " in diffs[0]
    with pytest.raises(AssertionError, match="1 differences in 1 of 3 blocks"):
        planref.assert_same(sample, bplans, plans, stream="unit")


@pytest.mark.parametrize("name", planref.BLOCK_FIELDS)
def test_comparer_reports_one_wrong_block_field(pkg, sample, name):
    wrong = list(sample)
    old = getattr(wrong[1], name)
    wrong[1] = replace(wrong[1], **{name: old + 1 if name == "frames" else old ^ 1})
    bplans, plans = _returned(pkg, wrong)
    diffs = planref.compare(sample, bplans, plans, stream="unit")
    assert len(diffs) == 1, diffs
    assert f"unit block 1 ({BLOCK} frames): {name} = {getattr(wrong[1], name)}, oracle {old}" in diffs[0]
    assert "probe margin ms - lr" in diffs[0]
    # a caller that narrows the block fields does not see it, the slots still count
    assert planref.compare(sample, bplans, plans, block_fields=tuple(f for f in planref.BLOCK_FIELDS if f != name)) == []


def test_comparer_reports_extra_and_missing_valid_slots(pkg, sample):
    bplans, plans = _returned(pkg, sample)
    spare = next(s for s in range(4) if s not in sample[0].slots)
    plans[spare].valid = 1  # e.g. left over from an earlier call
    diffs = planref.compare(sample, bplans, plans, stream="unit")
    assert len(diffs) == 1 and f"slot {spare} " in diffs[0] and "valid = 1, expected 0" in diffs[0], diffs
    plans[spare].valid = 0
    plans[2 * 16 + 7].valid = 1  # a probe slot of the small final block
    diffs = planref.compare(sample, bplans, plans, stream="unit")
    assert len(diffs) == 1 and "block 2 (3000 frames) slot 7 " in diffs[0], diffs
    plans[2 * 16 + 7].valid = 0
    for slot in (15, 4):  # the last and the first probe slot missing
        plans[16 + slot].valid = 0
        diffs = planref.compare(sample, bplans, plans, stream="unit")
        assert len(diffs) == 1 and f"block 1 ({BLOCK} frames) slot {slot} " in diffs[0] and "valid = 0, oracle 1" in diffs[0], diffs
        plans[16 + slot].valid = 1
    plans[2 * 16 + (2 if not sample[2].choose_ms else 0)].valid = 0  # a loser of the full comparison missing
    assert len(planref.compare(sample, bplans, plans)) == 1
    assert planref.compare(sample, bplans[:2], plans) != [] and planref.compare(sample, bplans, plans[:32]) != []


def test_open_records_still_pin_the_valid_set(pkg, oracle, sample):
    """records=False (the cheap expectation of the forced modes): fields are open, the valid set is not."""
    left, right = planrecipes.noise(2 * BLOCK + 3000, 16, 3)
    exp = planref.expected_stream(oracle, left, right, 1, records=False)
    assert all(sorted(b.slots) == [2, 3] and b.choose_ms == 1 and not b.uncertain for b in exp)
    bplans, plans = _returned(pkg, planref.expected_stream(oracle, left, right, 1))
    assert planref.compare(exp, bplans, plans) == []
    plans[16].valid = 1
    assert len(planref.compare(exp, bplans, plans)) == 1
    mono = planref.expected_stream(oracle, left, None, 0, records=False)
    assert all(sorted(b.slots) == [0] for b in mono)


def test_silent_block_is_the_documented_deviation(oracle):
    z = np.zeros(BLOCK, dtype=np.int32)
    b = planref.expected_block(oracle, z, z, 2)
    assert (b.uncertain, b.est_ms, b.choose_ms, sorted(b.slots)) == (1, 0, 0, [0, 1])
    b = planref.expected_block(oracle, z[:4096], z[:4096], 2)  # at <= 4096 frames the full comparison runs as ever
    assert (b.uncertain, b.choose_ms, sorted(b.slots)) == (1, 0, [0, 1, 2, 3])
    one = z.copy()
    one[-1] = 1
    assert sorted(planref.expected_block(oracle, z, one, 2).slots) == [0, 1] + list(range(4, 16))


@pytest.mark.parametrize("bits", [16, 24])
def test_recipes_cover_what_they_promise(bits):
    """The conditions the GPU tests assert before they touch the device, here on the oracle alone: cases a (every block
    probed; predictor types 0, 1, 2; fixed orders 0..4; LPC orders 4..12; partition orders 0..3; residual modes; ties and
    wide margins), b (pairs of very different cost) and d (the four classes of the estimate)."""
    planrecipes.check_coverage_a(planrecipes.expected("a", bits), bits)
    planrecipes.check_coverage_b(planrecipes.expected("b", bits))
    planrecipes.check_coverage_d(planrecipes.expected("d", bits))
    planrecipes.check_coverage_certain(planrecipes.expected("certain", bits, arg=len(planrecipes.expected("a", bits))))


def test_middle_window_starts_cover_both_parities_and_a_multiple_of_64():
    starts = {n: planref.slot_window(n, 8)[0] for n in planrecipes.FINAL_FRAMES if n > planref.FULL_COMPARE_LIMIT}
    assert {s % 2 for s in starts.values()} == {0, 1} and any(s % 64 == 0 for s in starts.values()), starts
