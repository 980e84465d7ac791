"""Decoder memory safety without a device: the lane code of the decode kernels (csrc/decode_core.h), compiled for the host
(tests/native/sim_decode.cpp) plain and with AddressSanitizer + UBSan, over lacmutate.py's corpus of damaged streams and
over all of lacgrammar.py, against the oracle's decoder (laco_decode_ex: version 3 and its own version-2 walk).

The rules (mutantjudge.py): 1 the verdict -- what the oracle accepts decodes to the oracle's samples (or is refused with
status 9 where a zigzag value reaches 2^30), what it refuses at block b is refused first at block b, and untouched blocks
keep their base's samples; 2 bounds -- no sanitizer report with every buffer at exactly the device path's size, and no
load further than the 25 bytes the comment at BitIn derives past the end of its block; 3 path independence -- lean trip
or never, 1 or 64 columns of lane memory, stream order or a shuffled gathered layout: same statuses, same samples.

Version-2 mutants, where the oracle refuses block b: one lane walks the stream, so the blocks before b must have decoded,
and those that end before the first changed byte must equal the base's (damage may decode and only fail later); the
blocks behind b are "not reached" (status 8) unless b only failed the bit-depth check, which runs after the walk."""
import collections
import os
import time

import numpy as np
import pytest

import dectwin
import lacgrammar as g
import lacmutate
import lacstreams
import mutantjudge
import twinbuild


@pytest.fixture(scope="module")
def judged(oracle, pkg):
    return mutantjudge.judge(oracle, pkg.lacx.stream_parse)


def test_verdicts_match_the_oracle(judged):
    """Rule 1 over the whole corpus; every mutant keeps a container stream_parse accepts."""
    records, failures, seconds = judged
    print("corpus: %d mutants, judged in %.1f s" % (len(records), seconds))
    assert not failures, "%d mutants:\n%s" % (len(failures), "\n".join(failures[:40]))
    assert len(records) == len(lacmutate.corpus(None))


def test_corpus_is_not_hollow(judged):
    """The conditions that keep the comparison from being hollow: size, the accepted share, both sides per mutator
    family, every status reached, few accepted-by-the-oracle-but-9 mutants."""
    records, _, _ = judged
    assert len(records) >= 20000
    share = sum(r.accepted for r in records) / len(records)
    print("accepted share: %.1f %%" % (100 * share))
    assert 0.15 <= share <= 0.60
    sides = collections.defaultdict(lambda: [0, 0])
    for r in records:
        sides[r.mutant.family][0 if r.accepted else 1] += 1
    print("accepted / refused per family:", dict(sides))
    assert set(sides) == set(lacmutate.FAMILIES)
    for family, (acc, ref) in sides.items():
        assert ref >= 50, family
        assert acc >= 50 or family in ("table", "trunc"), family
    codes = collections.Counter(r.code for r in records)
    print("the twin's answers by status:", sorted(codes.items()))
    for status in (1, 2, 3, 4, 5, 6, 9):
        assert codes[status] >= 20, status
    assert codes[7] >= 5
    nines = [r.mutant.name for r in records if r.verdict9]
    assert len(nines) <= 0.02 * len(records), nines
    assert any(m.base.startswith("v2:") for m in lacmutate.corpus(None))


def test_sanitized_twin_bounds_and_path_independence(judged):
    """Rules 2 and 3: the sanitized build over the whole corpus, four switch settings per mutant that vary every switch
    and every pair of switches (all eight over the corpus; all eight per stream for lacgrammar, below)."""
    records, _, _ = judged
    try:
        failures, worst, seconds = mutantjudge.sanitized(records)
    except RuntimeError as why:
        pytest.skip(str(why))
    print("sanitized twin: %d mutants x 4 settings in %.1f s, largest overshoot %d bytes (derived bound %d)"
          % (len(records), seconds, worst, mutantjudge.DERIVED_OVERSHOOT))
    assert not failures, "%d:\n%s" % (len(failures), "\n".join(failures[:20]))
    assert worst == 19, "the measured overshoot changed: update the comment at BitIn (decode_core.h) and DESIGN 6b"


def test_twin_pad_is_the_products():
    """The twin's payload pad is kDecodeTailPad of lacx_types.h -- the constant api_decode.cpp allocates and clears --
    and that constant covers the derived overshoot (a pad below the measured one is reported: next test)."""
    assert dectwin.tail_pad() >= mutantjudge.DERIVED_OVERSHOOT
    with open(os.path.join(twinbuild.CSRC, "lacx_types.h")) as f:
        assert "constexpr size_t kDecodeTailPad = %d;" % dectwin.tail_pad() in f.read()


def test_a_pad_below_the_overshoot_is_reported():
    """The sanitized twin does see a read past the payload: with 4 pad bytes instead of 128, a run of 0xFF up to the
    stream's last byte -- a long unary run into the pad -- reads beyond the allocation."""
    exe, why = dectwin.sanitized_exe()
    if exe is None:
        pytest.skip(why)
    lac = g.build("unary_5000").lac
    bad = lac[:-40] + b"\xff" * 40
    lines, rc, err = dectwin.run_sanitized([bad], pad=4, exe=exe, workers=1)
    assert rc != 0 and "heap-buffer-overflow" in err, err
    lines, rc, err = dectwin.run_sanitized([bad], exe=exe, workers=1)
    assert rc == 0 and lines[0].over > 4 and lines[0].status == [3]


@pytest.fixture(scope="module")
def grammar_lines():
    exe, why = dectwin.sanitized_exe()
    if exe is None:
        return None, why
    names = list(g.ALL_NAMES)
    streams = [g.build(n).lac for n in names] + [lacstreams.to_v2(g.build(n).lac) for n in g.V2_SUBSET]
    lines, rc, err = dectwin.run_sanitized(streams, exe=exe)
    assert rc == 0, err
    return dict(zip(names + ["v2:" + n for n in g.V2_SUBSET], lines)), ""


def _expect(s):
    want = [0] * len(s.frames)
    if s.status:
        want[s.bad_block] = s.status
    return want


@pytest.mark.parametrize("name", g.ALL_NAMES)
def test_grammar_case_through_every_path(name, grammar_lines):
    """Every lacgrammar case through the twin with all eight switch settings: the generator's statuses and samples, the
    same down the lean and the general trip, with 1 and 64 columns, in stream order and gathered."""
    s = g.build(name)
    first = None
    for setting in range(8):
        r = dectwin.decode(s.lac, never_lean=setting & 1, cols=64 if setting & 2 else 1, gathered=(setting >> 2) * 7)
        assert r.status.tolist() == _expect(s), (name, setting)
        assert r.over <= mutantjudge.DERIVED_OVERSHOOT
        if s.status == 0:
            assert np.array_equal(r.left, np.array(s.left, dtype=np.int64)), (name, setting)
            assert s.right is None or np.array_equal(r.right, np.array(s.right, dtype=np.int64)), (name, setting)
        first = first or r
    lines, why = grammar_lines
    if lines is None:
        pytest.skip(why)
    ln = lines[name]
    assert ln.same == 1 and ln.status == _expect(s) and ln.pcm_hash == dectwin.pcm_hash(s.lac, first)
    assert ln.over <= mutantjudge.DERIVED_OVERSHOOT


@pytest.mark.parametrize("name", g.V2_SUBSET)
def test_grammar_case_as_version_2(name, grammar_lines):
    s = g.build(name)
    v2 = lacstreams.to_v2(s.lac)
    for never_lean in (0, 1):
        r = dectwin.decode(v2, never_lean=never_lean, cols=64)
        assert not r.status.any()
        assert np.array_equal(r.left, np.array(s.left, dtype=np.int64))
        assert s.right is None or np.array_equal(r.right, np.array(s.right, dtype=np.int64))
    lines, why = grammar_lines
    if lines is None:
        pytest.skip(why)
    assert lines["v2:" + name].same == 1 and not any(lines["v2:" + name].status)


def test_oracle_decode_ex_reports_block_and_largest_value(oracle):
    """laco_decode_ex on the grammar: the refused block, ~0 (None) above block level, and the largest zigzag value --
    the generator's own count for valid streams; laco_decode keeps refusing version 2."""
    for name in ("unary_5000", "zero_run_escapes", "sweep_03", "stereo_mode_1_24bit"):
        s = g.build(name)
        left, right, bad, max_u = oracle.decode_ex(s.lac)
        assert np.array_equal(left, np.array(s.left, dtype=np.int64)) and bad is None and max_u == s.max_u, name
        l2, r2, bad, _ = oracle.decode_ex(lacstreams.to_v2(s.lac))
        assert np.array_equal(l2, left) and (right is None or np.array_equal(r2, right))
        with pytest.raises(RuntimeError):
            oracle.decode(lacstreams.to_v2(s.lac))
    assert oracle.decode_ex(b"LA\x03" + bytes(20))[2] is None
    mix = g.build("sweep_03")
    ent, pays = lacmutate._payloads(mix.lac)
    pays[5] = pays[5][:-1] + bytes([pays[5][-1] ^ 1])
    bad = lacmutate._rebuild(mix.lac, ent, pays)
    assert oracle.decode_ex(bad)[2] == 5 and oracle.decode_ex(lacstreams.to_v2(bad))[2] in (5, len(ent) - 1)
