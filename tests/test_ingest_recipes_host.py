"""The ingest corpus and its reference before a device is asked anything (tests/ingestrecipes.py): the reference against the
oracle's autocorrelation and stereo estimate and against plain Python-integer loops, the conditions the corpus promises,
and -- for every mistake an ingest kernel can make that the reference can be told to make -- the corpus stream that sees it."""
import numpy as np
import pytest

import ingestrecipes as R
import planref


@pytest.fixture(scope="module")
def exp(oracle):
    """name -> (Stream, Tables) over the corpus, computed once."""
    return {name: (st, R.expected(st, oracle)) for name, st in R.corpus().items()}


def _channels(st):
    if st.right is None:
        return [st.left]
    return [st.left, st.right, *planref.mid_side(st.left, st.right)]


def _used(st):
    return (0,) if st.right is None else ((0, 1), (2, 3), (0, 1, 2, 3))[st.stereo_mode]


def test_lag_tables_equal_the_oracles_autocorrelation(exp, oracle):
    """Every table the reference writes -- the whole-block slots in use and the twelve probe slots -- is the oracle's
    autocorr of the same samples; every other slot keeps the sentinel."""
    sent = R.sentinel_tables(1).acorr[0, 0]
    checked = 0
    for name, (st, t) in exp.items():
        chans = _channels(st)
        est = st.right is not None and st.stereo_mode == 2
        for b in range(st.blocks):
            nb = min(R.BLOCK, st.frames - b * R.BLOCK)
            for slot in range(R.SLOTS):
                c = slot & 3
                written = (slot < 4 and c in _used(st)) or (slot >= 4 and est and nb > R.LIMIT)
                if not written:
                    assert np.array_equal(t.acorr[b, slot], sent), (name, b, slot)
                    continue
                a, cnt = planref.slot_window(nb, slot)
                seg = chans[c][b * R.BLOCK + a:b * R.BLOCK + a + cnt]
                assert np.array_equal(t.acorr[b, slot], oracle.autocorr(seg)), (name, b, slot)
                checked += 1
    assert checked > 1000


def test_lag_sums_equal_plain_integer_loops_on_the_short_cases(exp):
    """The 12-bit split against the definition in Python integers: every block of at most 4113 frames, every window of the
    magnitude cases, and the alternating full-scale block whose lags no 64-bit intermediate may touch carelessly."""
    checked = 0
    for name, (st, t) in exp.items():
        if st.frames > 4113 and name not in ("alt_fs24", "impulses", "big_sums"):
            continue
        chans = [c.astype(np.int64) for c in _channels(st)]
        for c in _used(st):
            assert list(t.acorr[0, c]) == R.plain_lags(chans[c][:R.BLOCK]), (name, c)
            checked += 1
        if st.stereo_mode == 2 and st.right is not None and st.frames > R.LIMIT:
            nb = min(st.frames, R.BLOCK)
            for slot in range(4, R.SLOTS):
                a, cnt = planref.slot_window(nb, slot)
                assert list(t.acorr[0, slot]) == R.plain_lags(chans[slot & 3][a:a + cnt]), (name, slot)
    assert checked > 60


def test_sums_and_flags_equal_the_oracles_estimate(exp, oracle):
    """The twelve sums (the oracle's order is the kernel's: kind * 4 + channel, kinds raw / difference / anti-difference,
    channels L R M S -- R.ORACLE_SUM), est_ms and uncertain of every per-block-stereo block; the sentinel elsewhere."""
    sent = R.sentinel_tables(1).sums[0]
    blocks = 0
    for name, (st, t) in exp.items():
        for b in range(st.blocks):
            if st.right is None or st.stereo_mode != 2:
                assert np.array_equal(t.sums[b], sent), (name, b)
                assert (t.bplans[b]["est_ms"], t.bplans[b]["uncertain"]) == (0, 0)
                continue
            a = b * R.BLOCK
            o = oracle.stereo_estimate(st.left[a:a + R.BLOCK], st.right[a:a + R.BLOCK])
            assert [int(t.sums[b][i]) for i in range(12)] == [int(o.sums[R.ORACLE_SUM[i]]) for i in range(12)], (name, b)
            assert (int(t.bplans[b]["est_ms"]), int(t.bplans[b]["uncertain"])) == (int(o.choose_ms), int(o.uncertain)), (name, b)
            blocks += 1
    assert blocks > 80


def test_the_corpus_meets_its_own_conditions(exp):
    t = exp["alt_fs24"][1]
    assert t.acorr[0, 3, 0] > 1 << 61 and t.acorr[0, 3, 1] < -(1 << 61) and t.acorr[0, 3, 11] < -(1 << 61)
    assert all(int(v) > 1 << 32 for v in exp["big_sums"][1].sums[0])
    full = {int(v) for _, t in exp.values() for v in t.need_full}
    assert full == {0x0, 0x1, 0x3, 0xC, 0xF}, full
    probe = {int(v) for _, t in exp.values() for v in t.need_probe}
    assert probe == {0, 0xFFF0}
    # the decisions, each by name
    for name, want in (("zero_big", (0x3, 0, 1, 0)), ("zero_big_r1", (0x0, 0xFFF0, 1, None)), ("zero_small", (0xF, 0, 1, None)),
                       ("certain_lr", (0x3, 0, 0, 0)), ("certain_ms", (0xC, 0, 0, 1)), ("boundary_1pct", (0x0, 0xFFF0, 1, 0))):
        t = exp[name][1]
        got = (int(t.need_full[0]), int(t.need_probe[0]), int(t.bplans[0]["uncertain"]))
        assert got == want[:3], (name, got)
        if want[3] is not None:
            assert int(t.bplans[0]["choose_ms"]) == want[3], name
    # the 1 % rule is met with equality, and by nothing else
    st, t = exp["boundary_1pct"]
    _, unc, lr, ms, active = R.estimate([int(v) for v in t.sums[0]], st.frames)
    assert unc and not active and abs(lr - ms) == min(lr, ms) // 100 != 0
    # a silent block at the limit and one above it; uncertain small blocks; every length class
    lengths = {min(R.BLOCK, st.frames - b * R.BLOCK) for st, _ in exp.values() for b in range(st.blocks)}
    assert set(R.LENGTHS) <= lengths
    assert {st.blocks for st, _ in exp.values()} >= {1, 2, 3, 7, 8, 9, 17, 33}
    assert sorted(s.blocks for s in R.tables()) == [9, 14, 23]  # (no multiple of eight: the plain tail of xcd_slot)
    kinds = {(s.channels, s.mode, s.bit_depth) for ls in R.tables() for s in ls.streams}
    assert {(1, 0, 16), (2, 0, 24), (2, 1, 24), (2, 2, 16), (2, 2, 24)} <= kinds
    # validation: every promised place and order
    for depth in (16, 24):
        two = R.TILE * 2 + 8
        assert exp[f"bad_first{depth}"][1].bplans[0]["first_bad"] == 0
        assert exp[f"bad_last{depth}"][1].bplans[0]["first_bad"] == (two - 1) | 0x80000000
        assert exp[f"bad_seam{depth}"][1].bplans[0]["first_bad"] == R.TILE - 1
        assert exp[f"bad_seam_next{depth}"][1].bplans[0]["first_bad"] == R.TILE
        assert list(exp[f"bad_several{depth}"][1].badidx[0]) == [300, 100]
        assert exp[f"bad_several{depth}"][1].bplans[0]["first_bad"] == 300
        t = exp[f"bad_ms{depth}"][1]
        assert (t.bplans[0]["first_bad"], t.bplans[0]["choose_ms"], t.need_full[0]) == (5 | 0x80000000, 1, 0xC)
        t = exp[f"bad_block1_{depth}"][1]
        assert list(t.bplans["invalid"]) == [0, 1] and t.bplans[1]["first_bad"] == 49
    assert exp["bad_i24_d16"][1].bplans[0]["first_bad"] == 17 and not exp["wide_i24_d24"][1].bplans[0]["invalid"]
    # the proxy sums' 32-bit per-thread partials hold: 16 samples' zigzags stay below 2^30 in every valid stream
    for name, (st, t) in exp.items():
        if st.right is not None and not t.bplans["invalid"].any():
            s = (st.left.astype(np.int64) - st.right)
            assert np.abs(s).max() < 1 << 25, name


def test_every_named_fault_is_seen_by_a_corpus_stream(exp):
    """Each mistake switched on in the reference changes at least one word of a stream of the corpus; the stream is
    printed.  A fault nobody sees fails."""
    for fault, (text, names) in R.FAULTS.items():
        seen = None
        for name in names:
            st, true = exp[name]
            wrong = R.expect_stream(st, faults={fault})
            d = R.differences(true, wrong, name)
            if d:
                seen = (name, len(d), d[0])
                break
        assert seen, f"{fault} ({text}): no stream of {names} sees it"
        print(f"{fault}: {text} -- seen by {seen[0]} ({seen[1]} words, first: {seen[2]})")


def test_layout_variants_are_the_same_stream(exp):
    """Every layout and offset of the layout cases expects the words of the planar stream, and their bytes decode back to
    the same samples."""
    for name in ("lay2", "lay1"):
        base = exp[name][1]
        vs = R.layout_variants(name)
        assert len(vs) == 4 + 4 + 7 + 3
        for v in vs:
            assert not R.differences(base, R.expected(v), v.name) and R.expected(v).strict.all()
            raw = v.arrays()
            if v.layout == R.I16:
                back = np.frombuffer(raw[0], dtype="<i2").astype(np.int32).reshape(-1, v.channels)
            elif v.layout == R.I24:
                b3 = np.frombuffer(raw[0], dtype=np.uint8).reshape(-1, 3).astype(np.int32)
                back = (((b3[:, 0] | (b3[:, 1] << 8) | (b3[:, 2] << 16)) << 8) >> 8).reshape(-1, v.channels)
            else:
                back = np.stack([np.frombuffer(x, dtype="<i4") for x in raw], axis=1)
            assert np.array_equal(back[:, 0], v.left) and (v.right is None or np.array_equal(back[:, 1], v.right))
