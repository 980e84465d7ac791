"""The corpora of x87recipes.py without a device: that they hold what they promise (counted on operands, long double
results and oracle answers alone), that the host compile of csrc/x87.h equals long double on every element and the oracle
on every table, and that the oracle's answers on the signal tables are the reference's (pinned: refpin.py)."""
import numpy as np
import pytest

import refpin
import x87dev
import x87recipes as X

DEPTHS = (16, 24)


def test_operations_corpus_holds_every_class():
    c, want = X.ops_corpus(), X.ops_expected()
    assert c.n == 1 << 20
    counts = X.ops_class_counts(c, want)
    for name, count in counts.items():
        if name in X.IMPOSSIBLE_CLASSES:
            assert count == 0, f"a division that ties ({name}): x87recipes.py argues there is none"
        else:
            assert count >= X.MIN_CLASS_COUNT, f"{name}: {count} elements"


def test_host_x87_equals_long_double_on_the_operations_corpus():
    c = X.ops_corpus()
    X.compare_ops(c, X.ops_expected(), x87dev.host_ops(c), "host compile of x87.h")


@pytest.mark.parametrize("depth", DEPTHS)
def test_tables_reach_every_branch(oracle, depth):
    """On the oracle alone, and on the long double restatement that tells where k was clamped (itself held to the oracle
    on every table)."""
    ts = X.table_set(depth)
    assert ts.tables.shape[0] >= 2000
    sig = slice(0, ts.n_signal)
    hi = lo = 0
    for t in range(ts.tables.shape[0]):
        used, coef, h, l = X.levinson_long_double(ts.tables[t], 12)
        assert used == ts.used[t, 4] and np.array_equal(coef, ts.coef[t, 4]), ts.names[t]
        if t < ts.n_signal:
            hi, lo = hi + h, lo + l
    assert hi > 0 and lo > 0, "k clamped at +0.999 and at -0.999 among the signal tables"
    assert (ts.coef[sig] == 32767).any() and (ts.coef[sig] == -32768).any(), "Q15 saturation either way among the signal tables"
    assert (ts.tables[sig, 0] == 0).any(), "R[0] = 0 (clamped to 1)"
    if depth == 24:
        assert (ts.tables[sig, 0] > 1 << 61).any(), "R[0] > 2^61"
        assert (ts.tables[:, 0] == np.iinfo(np.int64).min).any()
    assert (ts.tables[:, 0] < 0).any()
    # no PCM of the 25-bit domain stops the recursion early; the synthetic tables stop at every order
    assert (ts.used[sig] == np.asarray(X.CANDS)[None, :]).all()
    assert set(np.unique(ts.used[:, 4])) == set(range(2, 13)), np.bincount(ts.used[:, 4], minlength=13)
    assert set(np.unique(ts.used[:, 0])) == {2, 3, 4}
    # candidate c is the order-12 solve stopped after c steps
    assert np.array_equal(ts.used, np.minimum(ts.used[:, 4:5], np.asarray(X.CANDS)[None, :]))
    # zeros above `used` and at index 0
    j = np.arange(13)[None, None, :]
    assert (ts.coef[(j > ts.used[:, :, None]) | (j == 0)] == 0).all()


@pytest.mark.parametrize("depth", DEPTHS)
def test_stopping_tables_stop_where_constructed(depth):
    ts = X.table_set(depth)
    first = ts.names.index("stop0")
    for k, r in enumerate(X.stopping_tables()):
        t = next(i for i in range(1, 13) if r[i] != 0) - 1
        assert ts.used[first + k, 4] == min(t + 2, 12), (k, t, ts.used[first + k])


@pytest.mark.parametrize("depth", DEPTHS)
def test_host_levinson_equals_oracle_on_every_table(depth):
    """levinson_candidates (host compile) on every table, at full length and at every short block's highest valid order."""
    ts = X.table_set(depth)
    n = ts.tables.shape[0]
    idx = np.arange(n)
    for mvo in (32, 12, 10, 8, 6, 4, 1, 0):
        used, coef = x87dev.host_levinson(ts.tables, np.full(n, mvo, np.int32))
        want_used, want_coef = X.expected_for_mvo(ts, idx, np.full(n, mvo))
        bad = (used != want_used).any(1) | (coef != want_coef).any((1, 2))
        assert not bad.any(), (mvo, [ts.names[i] for i in np.flatnonzero(bad)[:5]])


@pytest.mark.parametrize("depth", DEPTHS)
def test_placements_mix_every_wave(depth):
    """What the device test relies on: block counts that are no multiple of 16, full and partly filled workgroups, and in
    every wave with live lanes to speak of, lanes that stop at different orders beside lanes that run to 12; need_probe
    words with holes and all-zero ones; every stream shape and every short final block."""
    ts = X.table_set(depth)
    finals, shapes = set(), set()
    for pl in X.placements(depth):
        assert pl.blocks % 16 != 0 and pl.blocks * X.SLOTS > 256 and (pl.blocks * X.SLOTS) % 256 != 0
        lane = np.arange(pl.blocks * X.SLOTS)
        live = pl.written[lane % pl.blocks, lane // pl.blocks]
        used12 = ts.used[pl.table_idx[lane % pl.blocks, lane // pl.blocks], 4]
        for w in range(0, lane.size, 64):
            u = used12[w:w + 64][live[w:w + 64]]
            if u.size >= 8:
                assert (u == 12).any() and np.unique(u[u < 12]).size >= 2, (pl.name, w)
        assert (pl.need_probe == 0).any() and ((pl.need_probe & 0xFFF0) == 0xFFF0).any()
        assert any(0 < (int(w) & 0xFFF0) < 0xFFF0 for w in pl.need_probe)
        assert pl.written.any() and not pl.written.all()
        for frames, ch, sm in pl.streams:
            finals.add(frames - (X._stream_blocks(frames) - 1) * X.MAX_BLOCK)
            shapes.add((ch, sm))
        want = X.expected_lpcs(depth, pl)
        assert (want["pad"][pl.written] == 0).all()
    assert finals >= set(X.SHORT_FINALS) and shapes == {(1, 0), (2, 0), (2, 1), (2, 2)}
    short = [pl for pl in X.placements(depth) if pl.as_table and len(pl.streams) > 1]
    want = X.expected_lpcs(depth, short[0])
    assert (want["used"][short[0].written] == 0).any(), "a short final block skips candidates (mvo < cand)"
    probe_written = sum(int(pl.written[:, 4:].sum()) for pl in X.placements(depth))
    assert probe_written > 1000


@pytest.mark.parametrize("depth", DEPTHS)
def test_oracle_lpc_equals_reference_on_the_signals(oracle, depth):
    """LPC::levinson_durbin is private in the reference, so the tables as such cannot be pinned: the signals are."""
    ref = refpin.reference()
    for name, pcm in X.signals(depth):
        for cand in X.CANDS:
            u1, c1 = oracle.lpc_analyze(pcm, cand)
            u2, c2 = ref.lpc_analyze(pcm, cand)
            assert u1 == u2 and np.array_equal(c1, c2), (name, cand)
