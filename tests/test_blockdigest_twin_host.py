"""Block digests without a device: the CPU twin (tests/native/sim_blockdigest.cpp -- csrc/decode_plan.h's blocks form,
csrc/blockdigest_core.h summed as k_digest_blocks sums it with both trees and the straddle split, the judge and the
salvage pass, every buffer at exactly the plan's capacity; plain and under AddressSanitizer + UBSan as a program of its own)
against expectations that never come from the code under test: samples from the oracle block by block
(salvagetwin.expected), digests from zlib.crc32 over numpy-built data-chunk bytes, manifests from a restatement with struct."""
import collections
import glob
import os
import zlib

import numpy as np
import pytest

import blockdigesttwin as bt
import lacmutate
import lacstreams
import mutantjudge
import salvagetwin as st

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _read(path):
    with open(path, "rb") as f:
        return f.read()


FIXTURES = {os.path.basename(p)[:-4]: _read(p) for d in ("small", "decode_wav") for p in sorted(glob.glob(os.path.join(GOLDEN, d, "*.lac")))}


def _pcm(frames, depth, seed):
    rng = np.random.default_rng(seed)
    lim = 1 << (depth - 1)
    return rng.integers(-lim, lim, frames, dtype=np.int64).astype(np.int32)


# ---- unit level: the source form -----------------------------------------------------------------------------------
def _layouts(depth):
    names = ["planar_i32", "planar_f32", "inter_f32", "inter_i16" if depth == 16 else "inter_i24"] + (["planar_i16"] if depth == 16 else [])
    return [(n, bt.LAYOUTS[n]) for n in names]


def _offsets(name):
    """Every base offset a layout permits, counted from a 16-byte aligned address."""
    step = 1 if name == "inter_i24" else 2 if name == "planar_i16" else 4
    return range(0, 16, step)


GRIDS = (256, 257, 1000, 16384)


def _frame_counts(grid):
    out = {1, 3, 4, 5, grid - 1, grid, grid + 1, grid + 3, 2 * grid - 1, 2 * grid, 2 * grid + 2}
    return sorted(n for n in out if n >= 1)


@pytest.mark.parametrize("depth", [16, 24])
@pytest.mark.parametrize("channels", [1, 2])
def test_source_form_every_layout_offset_grid(channels, depth):
    """Every layout, channel count and depth at every base offset, in exact-size buffers, on grids 256, 257, 1000 and 16384
    with frame counts around the grid's multiples: every block's CRC-32 is zlib's over that block's bytes."""
    cases = 0
    for grid in GRIDS:
        counts = _frame_counts(grid) if grid < 16384 else [16383, 16384, 16385, 2 * 16384 + 1]
        for frames in counts:
            left, right = _pcm(frames, depth, frames * 7 + grid), _pcm(frames, depth, frames * 11 + grid + 1) if channels == 2 else None
            blocks = [min(grid, frames - a) for a in range(0, frames, grid)]
            want = [(n, c, 0) for n, c in zip(blocks, bt.block_crcs(left, right, depth, blocks))]
            for name, layout in _layouts(depth):
                offsets = _offsets(name) if grid < 16384 and frames <= grid + 3 else [0, 4 if name != "planar_i16" else 2]
                for off in offsets:
                    rows, key, atomics = bt.source_rows(layout, channels, depth, grid, off, left, right)
                    assert rows == want and key == bt.CLEAN, (name, grid, frames, off)
                    cases += 1
    print("source cases:", cases)


def test_full_block_costs_sixteen_atomics():
    """A 16384-frame block whose units start a workgroup: one atomic per workgroup, 16 in all; a straddled border adds the
    straddler's two pieces."""
    left = _pcm(16384, 16, 5)
    rows, _, atomics = bt.source_rows(bt.LAYOUTS["planar_i32"], 1, 16, 16384, 0, left)
    assert atomics == 16 and rows[0][1] == zlib.crc32(bt.data_bytes(left, None, 16))


def test_source_form_sanitized():
    """A selection of the unit-level cases as a program under AddressSanitizer + UBSan: no report, zlib's values."""
    exe, why = bt.sanitized_exe()
    if exe is None:
        pytest.skip(why)
    cases, wants = [], []
    for depth in (16, 24):
        for channels in (1, 2):
            for grid, frames in ((256, 255), (256, 257), (257, 516), (1000, 2001), (257, 1)):
                left, right = _pcm(frames, depth, frames + grid), _pcm(frames, depth, frames + grid + 9) if channels == 2 else None
                blocks = [min(grid, frames - a) for a in range(0, frames, grid)]
                want = ",".join("%d:%d:0" % (n, c) for n, c in zip(blocks, bt.block_crcs(left, right, depth, blocks)))
                for name, layout in _layouts(depth):
                    for off in _offsets(name):
                        cases.append(bt.source_case(layout, channels, depth, grid, off, left, right))
                        wants.append(want)
    lines, rc, err = bt.run_sanitized(cases, exe)
    assert rc == 0, err
    for i, (got, want) in enumerate(zip(lines, wants)):
        assert got is not None and got.split(" ", 1)[1] == "%d %s" % (bt.CLEAN, want), (i, got)


# ---- stream level -----------------------------------------------------------------------------------------------------
def _one_block(oracle, frames, channels, depth, seed):
    left = (_pcm(frames, depth, seed) >> 3).astype(np.int32)
    right = (_pcm(frames, depth, seed + 1) >> 3).astype(np.int32) if channels == 2 else None
    return oracle.encode(left, right, 48000, depth, 2 if channels == 2 else 0)


def _stitched(oracle):
    """name -> stream: three blocks of 257, 258 and 259 frames (seams at every residue mod 4), a final block of 1, 2 and 3
    frames, a one-frame stream; mono and stereo, 16 and 24 bit."""
    out = {}
    for channels in (1, 2):
        for depth in (16, 24):
            tag = "%dch%d" % (channels, depth)
            a, b, c = (_one_block(oracle, n, channels, depth, n) for n in (257, 258, 259))
            out["stitch|" + tag] = lacstreams.splice(lacstreams.splice(a, b), c)
            for tail in (1, 2, 3):
                out["tail%d|%s" % (tail, tag)] = lacstreams.splice(a, _one_block(oracle, tail, channels, depth, 40 + tail))
            out["one|" + tag] = _one_block(oracle, 1, channels, depth, 77)
    return out


@pytest.fixture(scope="module")
def streams(oracle):
    s = dict(lacmutate.bases(oracle.channel_block_end))
    s.update(FIXTURES)
    s.update(_stitched(oracle))
    for name in ("st16_lr_3blk", "mono16_16639"):
        s["v2|" + name] = lacstreams.to_v2(FIXTURES[name])
    return s


def test_clean_streams_rows_manifests_and_judge(oracle, streams):
    """The fixtures, the grammar bases, the stitched streams and version 2, as batches in all three forms: every row is
    zlib's, the manifest the twin's builder makes of them is the restatement's, and judged against it nothing is flagged."""
    names = sorted(streams)
    for at in range(0, len(names), 16):
        part = names[at:at + 16]
        lacs = [streams[n] for n in part]
        exps = [st.expected(oracle, x) for x in lacs]
        plain, _ = bt.run(lacs, None, bt.FORM_BLOCKS, cols=64 if at & 16 else 1)
        mans = []
        for name, lac, exp, it in zip(part, lacs, exps, plain):
            want = bt.expected_rows(exp, lac)
            assert it.code == 0, (name, it.message)
            for b, ((n, c, lost), row) in enumerate(zip(want, it.rows)):
                assert row[0] == n and (row[2] != 0) == lost and row[1] == c, (name, b, row, (n, c, lost))
            if any(lost for _, _, lost in want):
                mans.append(None)
                continue
            man = bt.manifest_for(exp, lac)
            crc = zlib.crc32(bt.data_bytes(exp.left, exp.right, lac[8]))
            assert bt.twin_manifest_build(lac[3], lac[8], st.rate(lac), exp.frames, crc, it.rows) == man, name
            mans.append(man)
        for form in (bt.FORM_BLOCKS, bt.FORM_WAV, bt.FORM_DEVICE):
            judged, _ = bt.run(lacs, mans, form, zero_status=form == bt.FORM_WAV)
            for name, lac, exp, it in zip(part, lacs, exps, judged):
                st.check("%s (form %d)" % (name, form), lac, exp, None, [r[2] for r in it.rows], st.result_of(it),
                         image=it.image, left=it.left, right=it.right)
                assert DIGEST_FREE(it.rows), name


def DIGEST_FREE(rows):
    return all(r[2] != bt.DIGEST for r in rows)


def test_a_manifest_of_another_stream_is_a_format_answer(oracle):
    lac, other = FIXTURES["st16_lr_3blk"], FIXTURES["mono16_16639"]
    man = bt.manifest_for(st.expected(oracle, other), other)
    items, _ = bt.run([lac, other, lac], [man, man, man[:-1]], bt.FORM_BLOCKS)
    assert items[0].code == 4 and items[0].message == "[check-error] channels: stream 2, manifest 1"
    assert items[1].code == 0 and items[2].code == 1 and items[2].message.startswith("[manifest-error] ")


# ---- the silent-damage corpus -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus(oracle, pkg):
    """Every version-3 mutant with its base's manifest: [(name, stream, the decode twin's statuses, base name)]."""
    records, failures, _ = mutantjudge.judge(oracle, pkg.lacx.stream_parse)
    assert not failures, failures[:5]
    return [(r.mutant.name, r.mutant.lac, r.status, r.mutant.base) for r in records if r.mutant.lac[2] == 3]


@pytest.fixture(scope="module")
def silent(oracle, corpus):
    """Every corpus entry through the plain twin, judged by its base's manifest, against the oracle: per entry (name,
    stream, manifest, the blocks expected with code 11, block frames)."""
    bases = lacmutate.bases(oracle.channel_block_end)
    base_info = {}
    for name in {b for _, _, _, b in corpus}:
        exp = st.expected(oracle, bases[name])
        base_info[name] = (bt.manifest_for(exp, bases[name]), exp)
    out, collisions = [], 0
    for at in range(0, len(corpus), bt.BATCH):
        part = corpus[at:at + bt.BATCH]
        k = at // bt.BATCH
        lacs = [lac for _, lac, _, _ in part]
        mans = [base_info[b][0] for _, _, _, b in part]
        wants = []
        for name, lac, status, base in part:
            exp2, wrong, hit = bt.judged_expectation(st.expected(oracle, lac), lac, base_info[base][1], bases[base])
            collisions += hit
            wants.append((exp2, wrong))
        form = (bt.FORM_WAV, bt.FORM_DEVICE, bt.FORM_BLOCKS)[k % 3]
        items, _ = bt.run(lacs, mans, form, cols=64 if k & 1 else 1, zero_status=bool(k & 2))
        for (name, lac, status, base), (exp2, wrong), man, it in zip(part, wants, mans, items):
            assert it.code == 0, (name, it.message)
            st.check("%s (form %d)" % (name, form), lac, exp2, status, [r[2] for r in it.rows], st.result_of(it),
                     image=it.image, left=it.left, right=it.right)
            out.append((name, lac, man, wrong, [r[0] for r in it.rows]))
    assert collisions == 0, "%d silently wrong blocks have their base's CRC-32" % collisions
    return out


def test_silent_damage_is_found_exactly(silent, corpus):
    """Code 11 on exactly the blocks the oracle decodes without fault to other bytes than the base's; lost blocks keep their
    codes, untouched blocks are never flagged, the output is the expectation with those blocks zeroed (the fixture
    asserts).  The corpus holds at least 10 000 mutants with such a block, at every length residue mod 4."""
    mutants = sum(1 for _, _, _, wrong, _ in silent if wrong)
    residues = collections.Counter(frames[b] % 4 for _, _, _, wrong, frames in silent for b in wrong)
    print("silent-damage corpus: %d streams, %d with a silently wrong block, %d such blocks, lengths mod 4: %s"
          % (len(silent), mutants, sum(residues.values()), sorted(residues.items())))
    assert len(silent) == len(corpus)
    assert mutants >= 10000
    assert all(residues[r] >= 1 for r in range(4))


def test_sanitized_twin_agrees_and_stays_inside_its_buffers(silent, streams, oracle):
    """A seeded selection of the corpus and every clean stream as a program of their own under AddressSanitizer + UBSan,
    all three forms: no report with every buffer at exactly the plan's capacity, and the plain build's answers."""
    exe, why = bt.sanitized_exe()
    if exe is None:
        pytest.skip(why)
    rng = np.random.default_rng(20261018)
    hit = [i for i, e in enumerate(silent) if e[3]]
    rest = [i for i, e in enumerate(silent) if not e[3]]
    pick = sorted(rng.choice(hit, 768, replace=False).tolist() + rng.choice(rest, 768, replace=False).tolist())
    lacs = [silent[i][1] for i in pick] + [streams[n] for n in sorted(streams)]
    mans = [silent[i][2] for i in pick] + [None] * len(streams)
    bt.cleared("selection", lacs, mans)
