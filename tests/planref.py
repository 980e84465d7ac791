"""What the device analysis must hand back for a stream, record by record, restated from the oracle, and the comparer
that holds `lacx_analyze`'s output against it.  Plain helper module (test infrastructure, no GPU, no test in here).

A block has sixteen slots: slot = window * 4 + channel, channels L R M S; window 0 is the whole block, windows 1..3 are
the 256-frame probe windows at 0, (n - 256) // 2 and n - 256 (ref lac/encoder.cpp:341-346).  The slots that must be
valid after an analysis:

  mono                                  slot 0                      ref lac/encoder.cpp:321-322
  forced left/right (stereo mode 0)     slots 0, 1                  ref lac/encoder.cpp:327-330
  forced mid/side (stereo mode 1)       slots 2, 3                  ref lac/encoder.cpp:323-326
  per block (mode 2), estimate certain  the estimated pair          ref lac/encoder.cpp:332-334, 364-371
  uncertain, n <= 4096                  slots 0..3 (both pairs are encoded and their sizes compared; the losers stay)
                                                                    ref lac/encoder.cpp:336-340
  uncertain, n > 4096                   slots 4..15 and the pair the probe sums pick (mid/side only when strictly
                                        smaller)                    ref lac/encoder.cpp:341-354
  uncertain, n > 4096, all zeros        slots 0, 1: the product's one deviation (csrc/k_front.hip, stereo_block) --
                                        twelve identical probe encodes tie, left/right stays, so no probe is run;
                                        `uncertain` stays 1, `choose_ms` 0

Every other slot must have `valid == 0`: the launch clears all plan records of the call's blocks with one memset before
the first kernel (csrc/k_analyze.hip, launch_analysis), and only a slot that was analysed writes its record, `valid = 1`
last (csrc/analyze_core.h).  A record left valid by an earlier call on the same handle would therefore show as an
extra valid slot.

`est_ms` / `uncertain` are the oracle's estimate (ref lac/encoder.cpp:126-197) in stereo mode 2 and 0 otherwise;
`choose_ms` is the final choice (1 for forced mid/side).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

BLOCK = 16384
PROBE = 256
FULL_COMPARE_LIMIT = 4096
SLOTS = 16
CHANNEL_NAMES = "LRMS"

BLOCK_FIELDS = ("frames", "invalid", "est_ms", "uncertain", "choose_ms")
SLOT_FIELDS = ("predictor_type", "order", "partition_order", "coef", "part_mode_k", "total_bits", "payload_bytes")


@dataclass(frozen=True)
class SlotRecord:
    predictor_type: int
    order: int
    partition_order: int
    coef: tuple            # coef[0..order) for LPC (predictor type 2), () otherwise
    part_mode_k: tuple     # (mode << 5) | k of every partition
    total_bits: int
    payload_bytes: int
    start: int = 0         # first frame of the slot's samples inside the block (for messages)
    n: int = 0             # frames of the slot


@dataclass(frozen=True)
class BlockRecord:
    frames: int
    invalid: int
    est_ms: int
    uncertain: int
    choose_ms: int
    slots: dict = field(default_factory=dict)  # slot number -> SlotRecord, exactly the slots that must be valid

    @property
    def margin(self):
        """ms_sum - lr_sum in bytes over the probe slots (None when the block is not probed)."""
        if not all(s in self.slots for s in range(4, SLOTS)):
            return None
        ms = sum(self.slots[s].payload_bytes for s in range(4, SLOTS) if (s & 3) >= 2)
        lr = sum(self.slots[s].payload_bytes for s in range(4, SLOTS) if (s & 3) < 2)
        return ms - lr


def mid_side(l, r):
    m = ((l.astype(np.int64) + r) >> 1).astype(np.int32)
    s = (l.astype(np.int64) - r).astype(np.int32)
    return m, s


def slot_window(frames: int, slot: int):
    """(first frame inside the block, frames) of a slot of a block of `frames` frames."""
    win = slot >> 2
    if win == 0:
        return 0, frames
    return (0, (frames - PROBE) // 2, frames - PROBE)[win - 1], PROBE


def slot_record(oracle, x, zr=True, pt=True, start=0, mask=0) -> SlotRecord:
    """The oracle's plan of one channel of one slot, in the fields of lacx_channel_plan.  mask != 0: of the search
    without the candidates of the mask (oracleshim.block_plan_encode_masked; the hooks library's LACX_DEBUG_SKIP bits 21..31)."""
    if mask:
        op, _, data = oracle.block_plan_encode_masked(x, zr, pt, mask)
        coef = tuple(int(op.coeffs_q15[i + 1]) for i in range(op.order)) if op.predictor_type == 2 else ()
        pmk = tuple((int(op.part_mode[i]) << 5) | int(op.part_k[i]) for i in range(op.part_count))
        return SlotRecord(int(op.predictor_type), int(op.order), int(op.partition_order), coef, pmk, int(op.total_bits),
                          len(data), start, int(np.asarray(x).size))
    op = oracle.block_plan(x, zr, pt)
    coef = tuple(int(op.coeffs_q15[i + 1]) for i in range(op.order)) if op.predictor_type == 2 else ()
    pmk = tuple((int(op.part_mode[i]) << 5) | int(op.part_k[i]) for i in range(op.part_count))
    return SlotRecord(int(op.predictor_type), int(op.order), int(op.partition_order), coef, pmk, int(op.total_bits),
                      len(oracle.block_encode(x, zr, pt)), start, int(np.asarray(x).size))


def wide_slot_record(oracle, x, zr=True, pt=True) -> SlotRecord:
    """slot_record for Block::Encoder's whole int32 domain (csrc/wide.hip).  `payload_bytes` is what the plan itself
    implies, (16 header bits + 16 per LPC coefficient + total_bits) >> 3, not the emitted length: at k = 31 the reference's
    estimate drops the quotient that its emit writes (csrc/api_encode.cpp, lacx_block_encode), so the two can differ
    there, and the emitted length is checked through the bytes themselves."""
    op = oracle.block_plan(x, zr, pt)
    coef = tuple(int(op.coeffs_q15[i + 1]) for i in range(op.order)) if op.predictor_type == 2 else ()
    pmk = tuple((int(op.part_mode[i]) << 5) | int(op.part_k[i]) for i in range(op.part_count))
    payload = (16 + (16 * int(op.order) if op.predictor_type == 2 else 0) + int(op.total_bits)) >> 3
    return SlotRecord(int(op.predictor_type), int(op.order), int(op.partition_order), coef, pmk, int(op.total_bits),
                      payload, 0, int(np.asarray(x).size))


def expected_block(oracle, l, r, stereo_mode, zr=True, pt=True, chosen_only=False, records=True, mask=0) -> BlockRecord:
    """The expectation of one block (r is None: mono).  chosen_only: only the pair (or the mono slot) that is emitted,
    which is all lacx_emit_from_plans needs.  records=False: a whole-block slot whose record decides nothing is expected
    valid but its fields are left open (None) -- the valid set and the block record without the oracle's most expensive
    plans.  mask: every slot's search without the candidates of the mask (slot_record); the probe sizes, and with them
    `choose_ms`, are those of the masked search."""
    n = int(l.size)
    if r is None:
        return BlockRecord(n, 0, 0, 0, 0, {0: slot_record(oracle, l, zr, pt, 0, mask) if records else None})
    m, s = mid_side(l, r)
    chans = (l, r, m, s)

    def rec(slot):
        a, cnt = slot_window(n, slot)
        return slot_record(oracle, chans[slot & 3][a:a + cnt], zr, pt, a, mask)

    est_ms = uncertain = 0
    slots = {}
    if stereo_mode in (0, 1):
        choose_ms = stereo_mode
    else:
        st = oracle.stereo_estimate(l, r)
        est_ms, uncertain = int(st.choose_ms), int(st.uncertain)
        choose_ms = est_ms
        if uncertain:
            if n <= FULL_COMPARE_LIMIT:
                slots = {c: rec(c) for c in range(4)}
                choose_ms = int(slots[2].payload_bytes + slots[3].payload_bytes <
                                slots[0].payload_bytes + slots[1].payload_bytes)
            elif not l.any() and not r.any():
                choose_ms = 0  # the documented deviation: no probes for digital silence, the tie keeps left/right
            else:
                slots = {c: rec(c) for c in range(4, SLOTS)}
                lr = sum(slots[c].payload_bytes for c in range(4, SLOTS) if (c & 3) < 2)
                ms = sum(slots[c].payload_bytes for c in range(4, SLOTS) if (c & 3) >= 2)
                choose_ms = int(ms < lr)
    pair = (2, 3) if choose_ms else (0, 1)
    if chosen_only:
        slots = {c: v for c, v in slots.items() if c in pair}
    for c in pair:
        if c not in slots:
            slots[c] = rec(c) if records else None
    return BlockRecord(n, 0, est_ms, uncertain, choose_ms, slots)


def expected_stream(oracle, left, right, stereo_mode, zr=True, pt=True, chosen_only=False, records=True, mask=0) -> list:
    """One BlockRecord per 16384-frame block of the stream."""
    out = []
    for a in range(0, int(left.size), BLOCK):
        out.append(expected_block(oracle, left[a:a + BLOCK], None if right is None else right[a:a + BLOCK], stereo_mode,
                                  zr, pt, chosen_only, records, mask))
    return out


def counts(expected):
    """(whole-block slots, probe slots) that must be valid: what lacx_timing's full_slots / probe_slots count."""
    full = sum(1 for b in expected for s in b.slots if s < 4)
    return full, sum(len(b.slots) for b in expected) - full


def to_ctypes(lacx, expected):
    """The expectation as the (lacx_block_plan[nb], lacx_channel_plan[nb * 16]) arrays of the C ABI."""
    nb = len(expected)
    bplans = (lacx.BlockPlan * nb)()
    plans = (lacx.ChannelPlan * (nb * SLOTS))()
    for b, blk in enumerate(expected):
        bp = bplans[b]
        bp.frames, bp.invalid, bp.est_ms, bp.uncertain, bp.choose_ms = (blk.frames, blk.invalid, blk.est_ms,
                                                                        blk.uncertain, blk.choose_ms)
        bp.first_bad = 0xFFFFFFFF
        for slot, r in blk.slots.items():
            dst = plans[b * SLOTS + slot]
            dst.predictor_type, dst.order, dst.partition_order, dst.valid = r.predictor_type, r.order, r.partition_order, 1
            for i, c in enumerate(r.coef):
                dst.coef[i] = c
            dst.total_bits = r.total_bits
            dst.payload_bytes = r.payload_bytes
            for i, v in enumerate(r.part_mode_k):
                dst.part_mode_k[i] = v
    return bplans, plans


def slot_diffs(pl, want: SlotRecord) -> list:
    """[(field, got, expected)] of a lacx_channel_plan that must be valid against the oracle's record: the one field list
    of every plan comparison in the suite."""
    out = []
    if pl.valid != 1:
        return [("valid", int(pl.valid), 1)]
    if want is None:  # expected valid, fields left open (expected_block, records=False)
        return out
    for name in ("predictor_type", "order", "partition_order", "total_bits", "payload_bytes"):
        if int(getattr(pl, name)) != getattr(want, name):
            out.append((name, int(getattr(pl, name)), getattr(want, name)))
    for i, c in enumerate(want.coef):
        if int(pl.coef[i]) != c:
            out.append((f"coef[{i}]", int(pl.coef[i]), c))
    for i, v in enumerate(want.part_mode_k):
        if int(pl.part_mode_k[i]) != v:
            out.append((f"part_mode_k[{i}]", int(pl.part_mode_k[i]), v))
    return out


def check_slot(pl, want: SlotRecord, what="plan"):
    d = slot_diffs(pl, want)
    assert not d, f"{what}: " + "; ".join(f"{n} = {g}, oracle {w}" for n, g, w in d)


def compare(expected, bplans, plans, stream="stream", block_fields=BLOCK_FIELDS) -> list:
    """Every difference between the expectation and what the analysis returned, as readable lines: stream, block, slot,
    channel and window start, field, both values.  Empty list: equal.  `block_fields` narrows the block record's fields
    (the valid set and all fields of the valid slots are always compared)."""
    out = []
    if len(bplans) != len(expected):
        return [f"{stream}: {len(bplans)} block records, expected {len(expected)}"]
    if len(plans) != len(expected) * SLOTS:
        return [f"{stream}: {len(plans)} slot records, expected {len(expected) * SLOTS}"]
    for b, want in enumerate(expected):
        bp = bplans[b]
        where = f"{stream} block {b} ({want.frames} frames)"
        for name in block_fields:
            if int(getattr(bp, name)) != getattr(want, name):
                extra = f" [probe margin ms - lr = {want.margin} bytes]" if want.margin is not None else ""
                out.append(f"{where}: {name} = {int(getattr(bp, name))}, oracle {getattr(want, name)}{extra}")
        for slot in range(SLOTS):
            pl = plans[b * SLOTS + slot]
            a, cnt = slot_window(want.frames, slot) if (slot < 4 or want.frames > FULL_COMPARE_LIMIT) else (0, 0)
            sw = f"{where} slot {slot} ({CHANNEL_NAMES[slot & 3]}, " + \
                 ("whole block" if slot < 4 else f"probe window {(slot >> 2) - 1} at frame {a}") + ")"
            if slot not in want.slots:
                if pl.valid != 0:
                    out.append(f"{sw}: valid = {int(pl.valid)}, expected 0 (not analysed for this block)")
                continue
            for name, got, exp in slot_diffs(pl, want.slots[slot]):
                out.append(f"{sw}: {name} = {got}, oracle {exp}")
    return out


def assert_same(expected, bplans, plans, stream="stream", block_fields=BLOCK_FIELDS, limit=40):
    d = compare(expected, bplans, plans, stream, block_fields)
    if d:
        blocks = len({line[len(stream):].split(" ")[2] for line in d if line.startswith(f"{stream} block ")})
        more = f"\n... and {len(d) - limit} more" if len(d) > limit else ""
        raise AssertionError(f"{len(d)} differences in {blocks} of {len(expected)} blocks:\n" + "\n".join(d[:limit]) + more)
