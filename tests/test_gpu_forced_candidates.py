"""Every predictor candidate of k_analyze<16,1024> and k_analyze<8,32> against the oracle, one at a time: the search of the
hooks library (liblacx_hooks.so) with candidates masked out by LACX_DEBUG_SKIP bits 21..31, against the oracle's search
with the same mask (tests/forcedrecipes.py says what a mask is, which two rules it obeys on both sides and how the masked
oracle is pinned without a GPU: tests/test_forced_candidates_host.py).  Exact equality everywhere, no case left out.

  a. whole blocks, one candidate each: the 112 blocks of the narrow corpus (4097..16384 samples) in corpus order on one
     `BlockEncoder` per mask, every plan field and every byte; all four flag pairs on the corpus' FLAG_SUBSET.  With one
     candidate in the search the winner is the candidate evaluated last: the residual and scans it left in LDS go
     straight to the partition search and the fused emit (11 x 112 runs of a path the unmasked corpus takes 9 times);
  b. short and ragged blocks: the 105 `geometry` blocks of the short corpus and all 143 blocks of 1..13 samples; the
     expectation states per block whether the mask applied, was ignored because the one order left does not exist for
     the block (LPC orders above n - 1), or had no effect because the block is silent;
  c. pairs: twelve frozen two-candidate masks -- ties (the lower index must win), the later and the earlier candidate of
     the reference's order winning by at most 0.5 % (forcedrecipes.PAIRS; ties exist in the corpus, none was built);
  d. probe geometry: planrecipes' case a (56 blocks, all probed, 16 and 24 bit) through `Encoder.analyze` under each
     single-candidate mask: the twelve probe records, the whole-block records and the block records, `choose_ms` as the
     masked probe sizes decide it;
  e. streams: the first stream of the narrow corpus (15 + 1 blocks per channel) through `Encoder.encode` under each
     single-candidate mask, forced left/right, forced mid/side and per block, with the fused emit and with k_emit alone;
  f. the plain siblings of the optimised paths: hook bits 128, 16384, 32768, 131072, 262144, 524288 and 1048576, each
     alone and all seven together, no mask, the whole narrow corpus against the unmasked oracle.  All seven preserve the
     plan (forcedrecipes' docstring gives the reading of each); none had to be left out.

The conditions the masked corpora meet are asserted on the oracle alone (forcedrecipes.check_coverage, cached) before the
device is asked anything.  The oracle's side of the module is about 10 s on the CPU (eight threads), shared through
forcedrecipes' caches.

Per-test GPU wall times, measured on an MI355X (111 cases, 11 s together, the oracle's side included): the cached
conditions 0.9 s once; a. a mask over the 112 blocks at most 0.09 s (the first one 0.28 s), over the flag subset 0.08 s;
b. 248 short blocks 0.13 s; c. four pairs 0.02 s; d. 56 probed blocks at most 0.22 s; e. three stereo modes twice, fused
0.06 s, k_emit alone 0.03 s; f. a hook bit over the corpus 0.11 .. 0.13 s (the first one 1.3 s more for the unmasked
expectation)."""
import pytest

import forcedrecipes as F
import narrowrecipes as N
import oracleshim as O
import planrecipes as P
import planref

pytestmark = pytest.mark.gpu

CAND = pytest.mark.parametrize("c", range(F.NC), ids=F.CANDIDATES)
RULE_TEXT = {O.MASK_APPLIED: "mask applied", O.MASK_NONE_LEFT: "mask ignored: no candidate left",
             O.MASK_SILENT: "silent: mask without effect"}


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lacx.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests need an MI355X (the product has no CPU fallback)")
    pkg.lacx.use_library(pkg.lacx.HOOKS_LIB_PATH)
    try:
        yield pkg
    finally:
        pkg.lacx.use_library(None)


@pytest.fixture(scope="module")
def covered():
    return F.check_coverage()


def _hook(monkeypatch, mask, extra=0):
    """LACX_DEBUG_SKIP is read when an encoder is created: set it first."""
    monkeypatch.setenv("LACX_DEBUG_SKIP", F.debug_skip(mask, extra))


def _walk(gpu, rows, zr=True, pt=True, what=""):
    """One handle for all the rows, in the order given: plan fields and bytes.  rows: (block, record, bytes, rule or None)."""
    be = gpu.lacx.BlockEncoder(12)
    be.set_zero_run_enabled(zr)
    be.set_partitioning_enabled(pt)
    bad = []
    try:
        for b, rec, data, rule in rows:
            where = f"{what}{b.family}/{b.name} (n = {b.x.size}, zero runs {zr}, partitions {pt}" + \
                    (f", {RULE_TEXT[rule]})" if rule is not None else ")")
            bad += [f"{where}: plan {name} = {got}, oracle {want}" for name, got, want in planref.slot_diffs(be.plan(b.x), rec)]
            got = be.encode(b.x)
            if got != data:
                first = next((i for i, (p, q) in enumerate(zip(got, data)) if p != q), min(len(got), len(data)))
                bad.append(f"{where}: {len(got)} bytes, oracle {len(data)}, first difference at byte {first}")
    finally:
        be._enc.close()
    assert not bad, f"{len(bad)} differences:\n" + "\n".join(bad[:40])
    return len(rows)


# -- a. whole blocks, one candidate each ---------------------------------------------------------------------------------

@CAND
def test_single_candidate_blocks_equal_the_oracle(gpu, covered, monkeypatch, c):
    _hook(monkeypatch, F.SINGLE[c])
    rows = [r for f in N.FAMILIES for r in F.expected(f, F.SINGLE[c])]
    assert _walk(gpu, rows, what=f"{F.CANDIDATES[c]} alone: ") == len(N.corpus())


@pytest.mark.parametrize("zr,pt", N.FLAGS[1:], ids=["no_partitions", "no_zero_runs", "neither"])
@CAND
def test_single_candidate_blocks_under_the_other_flag_pairs(gpu, covered, monkeypatch, c, zr, pt):
    _hook(monkeypatch, F.SINGLE[c])
    rows = [r for f in N.FLAG_SUBSET for r in F.expected(f, F.SINGLE[c], zr, pt)]
    assert _walk(gpu, rows, zr, pt, f"{F.CANDIDATES[c]} alone: ") == sum(len(N.family(f)) for f in N.FLAG_SUBSET)


# -- b. short and ragged blocks --------------------------------------------------------------------------------------------

@CAND
def test_single_candidate_short_blocks_equal_the_oracle(gpu, covered, monkeypatch, c):
    _hook(monkeypatch, F.SINGLE[c])
    rows = F.expected_short(F.SINGLE[c])
    assert {r.rule for r in rows} >= ({O.MASK_APPLIED, O.MASK_SILENT} | ({O.MASK_NONE_LEFT} if c >= 6 else set()))
    assert _walk(gpu, rows, what=f"{F.CANDIDATES[c]} alone: ") == len(F.short_blocks())


# -- c. pairs --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["tie", "later", "earlier"])
def test_two_candidate_searches_equal_the_oracle(gpu, covered, monkeypatch, kind):
    count = 0
    for k, a, b, mask, row in F.pair_rows():
        if k != kind:
            continue
        _hook(monkeypatch, mask)
        count += _walk(gpu, [row], what=f"{F.CANDIDATES[a]} and {F.CANDIDATES[b]} ({kind}): ")
    assert count == 4


# -- d. probe geometry -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", F.PROBE_BITS)
@CAND
def test_single_candidate_probe_and_block_records(gpu, monkeypatch, c, bits):
    _hook(monkeypatch, F.SINGLE[c])
    left, right = P.stream_a(bits)
    expected = F.expected_probes(bits, F.SINGLE[c])
    assert len(expected) == 56 and all(b.uncertain and b.margin is not None for b in expected)
    enc = gpu.lacx.Encoder(12, 2, F.RATE, bits, device=0)
    try:
        bplans, plans = enc.analyze(left, right)
        planref.assert_same(expected, bplans, plans, f"case a, {bits} bit, {F.CANDIDATES[c]} alone")
        t = enc.timing()
        assert (t.full_slots, t.probe_slots) == planref.counts(expected) == (2 * 56, 12 * 56)
    finally:
        enc.close()


def test_masks_move_the_stereo_choice(covered):
    """The masked probe sizes decide `choose_ms`: some block's choice differs from one mask to another (on the oracle
    alone; what the device makes of it is the test above)."""
    for bits in F.PROBE_BITS:
        choices = {tuple(b.choose_ms for b in F.expected_probes(bits, F.SINGLE[c])) for c in range(F.NC)}
        assert len(choices) > 1, bits


# -- e. streams through the fused emit ----------------------------------------------------------------------------------

@pytest.mark.parametrize("emit", ["fused", "k_emit_only"])
@CAND
def test_single_candidate_stream_bytes(gpu, monkeypatch, c, emit):
    """The fused emit takes its residual from what the last evaluated candidate left in LDS: with one candidate in the
    search that is this candidate, on every channel block of the stream."""
    _hook(monkeypatch, F.SINGLE[c])
    if emit == "k_emit_only":
        monkeypatch.setenv("LACX_FUSED_EMIT", "0")
    name, bits, left, right = F.stream()
    for mode in F.STREAM_MODES:
        want = F.stream_bytes(F.SINGLE[c], mode)
        enc = gpu.lacx.Encoder(12, mode, F.RATE, bits, device=0)
        try:
            for call in range(2):
                assert enc.encode(left, right) == want, (name, F.CANDIDATES[c], mode, emit, call)
        finally:
            enc.close()


# -- f. plain siblings of the optimised paths ---------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [(b,) for b in F.SIBLING_BITS] + [F.SIBLING_BITS],
                         ids=[f"bit_{b}" for b in F.SIBLING_BITS] + ["all_seven"])
def test_plain_siblings_equal_the_unmasked_oracle(gpu, monkeypatch, bits):
    _hook(monkeypatch, 0, sum(bits))
    rows = [(b, rec, data, None) for f in N.FAMILIES for b, rec, data in N.expected(f)]
    assert _walk(gpu, rows, what=f"hook bits {sum(bits)}: ") == len(N.corpus())
