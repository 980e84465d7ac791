"""tests/lacinspect.py pinned before anything is held against it: the header fields it reads out of every stream the oracle
encoded equal the oracle's own plan of that channel's PCM, every case of the block grammar gets its declared verdict, the
identities of the issue hold on every block that parses, and the corpus taken together is not hollow."""
import numpy as np

import inspectcorpus as ic
import lacinspect as li


def _pin_headers(oracle, name, lac, zr=True, pt=True):
    """Every channel block's predictor, order, coefficients, partition order and partition table against
    oracleshim.block_plan of that channel's PCM: left / right, or mid / side where the block is mid/side."""
    rows = ic.expected(lac)
    left, right, bad, _ = oracle.decode_ex(lac)
    assert left is not None and bad is None, name
    at = 0
    for b, row in enumerate(rows):
        assert row["code"] == 0, (name, b, row["code"])
        li.check_identities(row, ic.stereo_flag(lac))
        n = row["frames"]
        chans = [left[at:at + n]] if right is None else list(ic.mid_side(left[at:at + n], right[at:at + n]) if row["ms"] else (left[at:at + n], right[at:at + n]))
        assert row["channels"] == len(chans)
        for c, x in enumerate(chans):
            plan, got = oracle.block_plan(x, zr, pt), row["ch"][c]
            where = (name, b, c)
            assert (got["predictor_type"], got["order"], got["partition_order"]) == (plan.predictor_type, plan.order, plan.partition_order), where
            order = plan.order if plan.predictor_type == 2 else 0  # (the oracle's list is 1-based: a[1..order])
            assert got["coef"][:order] == list(plan.coeffs_q15)[1:order + 1] and not any(got["coef"][order:]), where
            assert [mk for mk, _ in got["partitions"]] == [(plan.part_mode[p] << 5) | plan.part_k[p] for p in range(plan.part_count)], where
        at += n
    return rows


def test_headers_of_encoded_streams_equal_the_oracles_plans(oracle):
    seen_final = set()
    count = 0
    for name, lac in ic.small() + ic.pinned() + ic.narrow(oracle):
        rows = _pin_headers(oracle, name, lac)
        seen_final.add(rows[-1]["frames"])
        count += len(rows)
    print("blocks pinned against the oracle's plans:", count)
    assert 1 in seen_final


def test_grammar_cases_get_their_declared_verdict():
    """Status 0 stays 0; 5 (sample overflow) and 7 (outside the bit depth) need samples and parse; every other status is the
    code of the block that breaks the rule, and the identities hold on every block that parses."""
    finals = set()
    for name, lac, status, bad_block in ic.grammar():
        rows = ic.expected(lac)
        want = 0 if status in (0, 5, 7) else status
        codes = [r["code"] for r in rows]
        if want == 0:
            assert not any(codes), (name, codes)
        else:
            assert codes[bad_block] == want, (name, codes)
            assert all(c in (0, 8) for k, c in enumerate(codes) if k != bad_block), (name, codes)
        for r in rows:
            if r["code"] == 0:
                li.check_identities(r, ic.stereo_flag(lac))
        finals.add(rows[-1]["frames"])
    assert 13 in finals or 13 in {ic.expected(l)[-1]["frames"] for _, l in ic.small() + ic.pinned()}, sorted(finals)[:20]


def test_the_corpus_is_not_hollow(oracle):
    chans, met = [], set()
    for lac in [l for _, l in ic.small() + ic.pinned() + ic.narrow(oracle)] + [l for _, l, _, _ in ic.grammar()]:
        met |= ic.seen(lac)
        for r in ic.expected(lac):
            chans += r["ch"][:r["channels"]] if r["code"] == 0 else []
    preds = {(c["predictor_type"], c["order"]) for c in chans}
    assert {(0, o) for o in range(5)} | {(1, 2)} <= preds
    lpc = {o for t, o in preds if t == 2}
    assert any(o <= 12 for o in lpc) and any(12 < o < 32 for o in lpc) and 32 in lpc, sorted(lpc)
    assert {c["partition_order"] for c in chans} == set(range(9))
    for m in range(4):
        assert ("mode", m, "block") in met and ("mode", m, "partition") in met, (m, met)
    assert {"stateful_run", "stateless_run", "run_ends_partition", "long_unary"} <= met, met
    assert any(c["escape_samples"] for c in chans)
    assert all(any(c["bin_samples"][t] for c in chans) for t in range(3))
    assert max(c["unary_max"] for c in chans) > 64


def test_report_totals():
    name, lac = ic.pinned()[0]
    rows = ic.expected(lac)
    t = li.report(rows, (lac[2], lac[3], lac[4], 48000, lac[8], len(rows)))
    assert t["frames"] == sum(r["frames"] for r in rows) and 8 * t["payload_bytes"] == t["flag_bits"] + t["bits"]
    assert sum(t[k] for k in li.BIT_CLASSES) == t["bits"] and sum(t["mode_samples"]) == t["frames"] * lac[3]
    assert t["head_bytes"] + t["payload_bytes"] == len(lac)
    assert np.sum(t["fixed_blocks"]) + t["fir_blocks"] + np.sum(t["lpc_blocks"]) == t["channel_blocks"] == sum(t["partition_order_blocks"])
