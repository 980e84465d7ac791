"""The rules a damaged stream is judged by (tests/lacmutate.py's corpus), shared by the host test and the device test:
the CPU twin of the decoder's lane code (dectwin.py) against the oracle's decoder (laco_decode_ex, version 3 and 2).

  judge(oracle, stream_parse)   every mutant through the oracle and the plain twin: rule 1 (the verdict), per mutant a
                                Record; the failures as text
  judge_list(...)               the same for any list of mutants (the device tests' own streams)
  cleared(oracle, parse, ...)   what may go to a device: records that passed rules 1-3 in this run, else AssertionError
  check_stream(lacx, ...)       mutants of a test's own stream: cleared, then through lacx.decode on the device
  sanitized(records)            every mutant through the sanitized twin, four switch settings each that vary every switch
                                and every pair of them (all eight over the corpus, dectwin.HALF_SETTINGS): rules 2 (no report,
                                overshoot <= DERIVED_OVERSHOOT) and 3 (path independence); the failures as text
"""
from __future__ import annotations

import time
from collections import namedtuple

import numpy as np

import dectwin
import lacgrammar
import lacmutate

DERIVED_OVERSHOOT = 25   # bytes: the figure the comment at BitIn (csrc/decode_core.h) derives
LIMIT = 1 << 30          # zigzag values from here on are refused by the device decoder (status 9)

# accepted: the oracle decodes it (left / right: its PCM); bad: the block the oracle refuses; status: the twin's per block;
# block / code: the twin's lowest failing block and its status (None, 0 where all decoded); verdict9: the oracle accepts
# a value >= 2^30 and the twin answers 9
Record = namedtuple("Record", "mutant accepted left right bad max_u status block code verdict9 pcm_hash over")

_cache = {}


def base_pcm(oracle, name, lac):
    key = ("base", name)
    if key not in _cache:
        left, right, bad, _ = oracle.decode_ex(lac)
        assert left is not None, "base %s does not decode (block %r)" % (name, bad)
        _cache[key] = (left, right)
    return _cache[key]


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and np.array_equal(a, b))


def _verdict(oracle, m, base, rec_left, rec_right, bad, max_u, tw):
    """Rule 1 for one mutant: '' or what is wrong."""
    st = tw.status
    nz = np.flatnonzero(st)
    version, ent, head = lacmutate.table(m.lac)
    edges = np.concatenate([[0], np.cumsum([n for n, _ in ent])])
    if rec_left is not None:
        if nz.size == 0:
            return "" if _same(tw.left, rec_left) and _same(tw.right, rec_right) else "PCM differs from the oracle's"
        if max_u >= LIMIT and st[nz[0]] == 9:
            return ""
        return "the oracle accepts (largest value %d), the twin says %d at block %d" % (max_u, st[nz[0]], nz[0])
    if bad is None:
        return "the oracle refuses above block level"
    if nz.size == 0 or nz[0] != bad:
        return "the oracle refuses block %d, the twin's statuses are %s" % (bad, st.tolist()[:40])
    bl, br = base_pcm(oracle, m.base, base)
    if version == 3:  # a refused block must not disturb others
        for b in lacmutate.unchanged_blocks(base, m.lac):
            a, e = edges[b], edges[b + 1]
            if st[b] != 0 or not np.array_equal(tw.left[a:e], bl[a:e]) or (br is not None and not np.array_equal(tw.right[a:e], br[a:e])):
                return "untouched block %d: status %d or samples differ from the base's" % (b, st[b])
        return ""
    # version 2: one lane walks the stream.  Blocks before the refused one decoded; those that end before the first
    # changed byte are the base's; the blocks behind it are not reached (unless it only failed the bit-depth check,
    # which runs after the walk)
    if st[bad] != 7 and any(s != 8 for s in st[bad + 1:]):
        return "version 2: blocks behind the refused one are not all 'not reached': %s" % st.tolist()[:40]
    same = next((i for i in range(min(len(base), len(m.lac))) if base[i] != m.lac[i]), min(len(base), len(m.lac)))
    v3 = _cache["bases"][m.base[3:]]  # a version-2 base "v2:<name>" is the rewrite of the version-3 base <name>
    _, ent3, _ = lacmutate.table(v3)
    end = head
    for b in range(bad):
        end += ent3[b][1]
        a, e = edges[b], edges[b + 1]
        if end <= same and not (np.array_equal(tw.left[a:e], bl[a:e]) and (br is None or np.array_equal(tw.right[a:e], br[a:e]))):
            return "version 2: block %d lies before the damage and differs from the base's" % b
    return ""


def judge_list(oracle, stream_parse, mutants, bases):
    """Rule 1 for each of `mutants` (their bases by name in `bases`) -> (records, failures)."""
    _cache.setdefault("bases", {}).update(bases)
    records, failures = [], []
    for m in mutants:
        if stream_parse(m.lac) is None:  # every mutator leaves a container the parser takes
            failures.append("%s: stream_parse refuses it" % m.name)
            continue
        left, right, bad, max_u = oracle.decode_ex(m.lac)
        tw = dectwin.decode(m.lac)
        why = _verdict(oracle, m, bases[m.base], left, right, bad, max_u, tw)
        if why:
            failures.append(m.name + ": " + why)
        nz = np.flatnonzero(tw.status)
        block, code = (int(nz[0]), int(tw.status[nz[0]])) if nz.size else (None, 0)
        records.append(Record(m, left is not None, left, right, bad, max_u, tw.status, block, code,
                              left is not None and code == 9, dectwin.pcm_hash(m.lac, tw), tw.over))
    return records, failures


def judge(oracle, stream_parse):
    """The whole corpus -> (records, failures, seconds)."""
    if "judge" not in _cache:
        t0 = time.time()
        records, failures = judge_list(oracle, stream_parse, lacmutate.corpus(oracle.channel_block_end),
                                       lacmutate.bases(oracle.channel_block_end))
        _cache["judge"] = (records, failures, time.time() - t0)
    return _cache["judge"]


def sanitized(records, key="san"):
    """-> (failures, largest overshoot, seconds), or raises RuntimeError where the sanitized twin cannot be built."""
    if key in _cache:
        return _cache[key]
    exe, why = dectwin.sanitized_exe()
    if exe is None:
        raise RuntimeError(why)
    t0 = time.time()
    lines, rc, err = dectwin.run_sanitized([r.mutant.lac for r in records], settings=dectwin.HALF_SETTINGS, exe=exe)
    failures = []
    if rc != 0:
        first = next((r.mutant.name for r, ln in zip(records, lines) if ln is None), "?")
        failures.append("the sanitized twin stopped (exit %d), first stream without an answer: %s\n%s" % (rc, first, err))
    worst = 0
    for r, ln in zip(records, lines):
        if ln is None:
            continue
        worst = max(worst, ln.over)
        if ln.over > DERIVED_OVERSHOOT:
            failures.append("%s: a load reached %d bytes past its block (derived bound: %d)" % (r.mutant.name, ln.over, DERIVED_OVERSHOOT))
        if not ln.same:
            failures.append("%s: the switch settings (lean policy, columns, layout) do not agree" % r.mutant.name)
        if ln.status != r.status.tolist() or ln.pcm_hash != r.pcm_hash:
            failures.append("%s: the sanitized build and the plain build differ" % r.mutant.name)
    _cache[key] = (failures, worst, time.time() - t0)
    return _cache[key]


def cleared(oracle, stream_parse, mutants=None, bases=None, key="san"):
    """The records of the corpus (or of `mutants`), after the sanitized twin has shown in this run that every one of them
    stays inside its buffers down every path.  Fails -- never skips -- where that cannot be shown."""
    if mutants is None:
        records, failures, _ = judge(oracle, stream_parse)
    else:
        records, failures = judge_list(oracle, stream_parse, mutants, bases)
    assert not failures, "rule 1 (verdict):\n" + "\n".join(failures[:20])
    try:
        failures, _, _ = sanitized(records, key)
    except RuntimeError as why:
        raise AssertionError("the sanitized twin is not available, nothing goes to the device unchecked: %s" % why)
    assert not failures, "rules 2 / 3 (bounds, paths):\n" + "\n".join(failures[:20])
    return records


def message(record):
    """The whole error text the device gives for a refused mutant: the twin's lowest failing block and its status."""
    return "[decode-error] block=%d %s" % (record.block, lacgrammar.STATUS_TEXT[record.code])


def check_stream(lacx, oracle, name, lac, families=("flip", "run", "trunc", "table")):
    """Mutants of any version-3 stream (a device test's own), cleared on the CPU, then through lacx.decode: refused exactly
    as the twin refuses them, or decoded to the oracle's samples.  Returns (decoded, refused)."""
    muts = [lacmutate.Mutant("%s|%s|%s" % (name, fam, par), name, fam, m)
            for fam, par, m in lacmutate.mutants_of(name, lac, oracle.channel_block_end) if fam in families and m != lac]
    recs = cleared(oracle, lacx.stream_parse, muts, {name: lac}, key="san:" + name)
    done = [0, 0]
    for r in recs:
        if r.code:
            try:
                lacx.decode(r.mutant.lac)
                text = "decoded"
            except RuntimeError as err:
                text = str(err)
            assert text == message(r), (r.mutant.name, text)
        else:
            left, right, _, _ = lacx.decode(r.mutant.lac)
            assert np.array_equal(left, r.left) and (r.right is None or np.array_equal(right, r.right)), r.mutant.name
        done[1 if r.code else 0] += 1
    return tuple(done)
