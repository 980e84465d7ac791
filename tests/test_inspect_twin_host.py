"""Stream inspection without a device: the CPU twin (tests/native/sim_inspect.cpp -- csrc/inspect_plan.h's job, the lanes of
csrc/inspect_core.h, csrc/inspect_rows.h's host side, every buffer at exactly the plan's capacity; plain and under
AddressSanitizer + UBSan as a program of its own) against tests/lacinspect.py, bit for bit, and over the whole mutation
corpus against the decode twin block by block."""
import random

import inspectcorpus as ic
import inspecttwin as tw
import lacinspect as li
import lacmutate
import mutantjudge


def _streams(oracle):
    return [l for _, l in ic.small() + ic.pinned() + ic.narrow(oracle)] + [l for _, l, _, _ in ic.grammar()]


def _same(got, lac, partitions):
    want = ic.expected(lac)
    assert got == (want if partitions else li.strip_partitions(want))


def test_rows_equal_the_reference_one_stream_at_a_time(oracle):
    """Every stream of every corpus as a batch of one, with partition detail: rows, partition entries and the report."""
    for lac in _streams(oracle):
        rc, rows, reps, over = tw.run([lac], partitions=True, cols=64)
        assert rc == [0] and over <= 25
        _same(rows[0], lac, True)
        assert reps[0] == li.report(ic.expected(lac), (lac[2], lac[3], lac[4], lac[6] | (lac[5] << 8) | (lac[7] << 16), lac[8], len(rows[0])))


def test_rows_equal_the_reference_in_shuffled_batches(oracle):
    """Batches with duplicates, refused containers among them, with and without partition detail, wave padding on and off."""
    lacs = _streams(oracle)
    rng = random.Random(5)
    for trial in range(4):
        pick = [rng.choice(lacs) for _ in range(60)]
        pick[7], pick[31] = b"LA\x03", pick[3][:13]  # refused: they get no rows, the others are not disturbed
        partitions = bool(trial & 1)
        rc, rows, reps, _ = tw.run(pick, partitions=partitions, cols=1 if trial < 2 else 64, pad_waves=trial == 3)
        for i, lac in enumerate(pick):
            if i in (7, 31):
                assert rc[i] != 0 and rows[i] is None and not any(v for v in reps[i].values() if not isinstance(v, list))
                continue
            assert rc[i] == 0
            _same(rows[i], lac, partitions)


def test_cut_streams_report_their_missing_blocks(oracle):
    """A version-3 file cut at every kind of place: the blocks it holds as before, code 10 with frames and bytes for the rest."""
    count = 0
    for name, lac in ic.pinned() + ic.narrow(oracle)[:2]:
        if lac[2] != 3:
            continue
        whole = ic.expected(lac)
        for cut in ic.cuts(lac):
            rc, rows, _, _ = tw.run([cut], partitions=True)
            assert rc == [0]
            _same(rows[0], cut, True)
            codes = [r["code"] for r in rows[0]]
            assert 10 in codes and codes == sorted(codes, key=lambda c: c == 10), codes
            assert all(r == w for r, w in zip(rows[0], whole) if r["code"] != 10)
            count += 1
    assert count > 50


def test_path_independence(oracle):
    """1 or 64 columns of lane memory, stream order or a gathered layout: the same rows."""
    for lac in _streams(oracle):
        if lac[2] != 3:
            continue
        want = tw.run([lac], partitions=True, cols=1)[1][0]
        for cols, seed in ((64, 0), (1, 7), (64, 13)):
            assert tw.run([lac], partitions=True, cols=cols, gather_seed=seed)[1][0] == want


def test_sanitized_twin_clears_the_corpora(oracle):
    """The stand-alone sanitized program over every corpus in batches, buffers at exactly the plan's capacities: no report,
    and the plain build's answers."""
    lacs = _streams(oracle)
    lacs += [c for _, l in ic.pinned() if l[2] == 3 for c in ic.cuts(l)]
    assert tw.cleared("corpora", lacs) == lacs


def test_mutation_corpus_against_the_decode_twin(oracle, pkg):
    """Every block of every mutant: decode status 0 or 7 -> 0; 1 2 3 4 6 9 -> the same code; 8 behind a parse fault -> 8.
    Decode status 5, and the blocks behind such a block in a version-2 stream, are judged by lacinspect.py instead (the
    parse goes on where the synthesis stopped): that class stays at or below 5 % of the corpus's blocks."""
    records, _, _ = mutantjudge.judge(oracle, pkg.lacx.stream_parse)  # the decode twin's statuses, computed once per run
    corpus = [r.mutant for r in records]
    assert len(corpus) == len(lacmutate.corpus(oracle.channel_block_end))
    lacs = [m.lac for m in corpus]
    got = []
    for at in range(0, len(lacs), 512):
        got += tw.codes(lacs[at:at + 512], cols=64 if (at // 512) & 1 else 1)[0]
    blocks = by_reference = 0
    for r, codes in zip(records, got):
        m = r.mutant
        assert codes is not None, m.name
        status = r.status.tolist()
        assert len(status) == len(codes)
        blocks += len(codes)
        open_from = None  # version 2: from a status-5 block on, the decode verdict does not determine the answer
        if 5 in status:
            open_from = status.index(5) if m.lac[2] == 2 else None
            want = [r["code"] for r in ic.expected(m.lac)]
        for b, (s, c) in enumerate(zip(status, codes)):
            if s == 5 or (open_from is not None and b > open_from):
                by_reference += 1
                assert c == want[b], (m.name, b, s, c, want[b])
            else:
                assert c == (0 if s in (0, 7) else s), (m.name, b, s, c)
    print("mutants %d, blocks %d, judged by the reference %d (%.2f %%)" % (len(corpus), blocks, by_reference, 100.0 * by_reference / blocks))
    assert by_reference * 20 <= blocks
