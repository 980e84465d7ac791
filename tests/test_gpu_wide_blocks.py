"""Block::Encoder outside the 25-bit domain (csrc/wide.hip, k_wide_block) against the oracle over the constructed corpus
of tests/widerecipes.py: for every block `BlockEncoder.plan` equals the oracle's record field by field (predictor type,
order, partition order, coefficients, every partition's mode and k, total_bits, payload_bytes) and `BlockEncoder.encode`
gives the oracle's bytes.  Exact equality everywhere, no block left out.

`payload_bytes` is compared with what the oracle's *plan* implies (planref.wide_slot_record): at k = 31 the reference's
estimate and its emit disagree, so the emitted length can exceed it and is checked through the bytes.  The conditions the
corpus meets are asserted on the oracle alone in tests/test_wide_blocks_host.py; the family `edge` holds twins on either
side of the dispatch edge |x| > 2^24, both members of which are compared here (the narrow one takes the streaming kernels).
"""
import pytest

import planref
import widerecipes as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lacx.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests need an MI355X (the product has no CPU fallback)")
    return pkg


def _block_encoder(gpu, zr=True, pt=True):
    be = gpu.lacx.BlockEncoder(12)
    be.set_zero_run_enabled(zr)
    be.set_partitioning_enabled(pt)
    return be


def _diffs(be, x, rec, data, what):
    """Plan and bytes of one block against the oracle, as readable lines."""
    out = [f"{what}: plan {name} = {got}, oracle {want}" for name, got, want in planref.slot_diffs(be.plan(x), rec)]
    got = be.encode(x)
    if got != data:
        first = next((i for i, (a, b) in enumerate(zip(got, data)) if a != b), min(len(got), len(data)))
        out.append(f"{what}: {len(got)} bytes, oracle {len(data)}, first difference at byte {first}")
    return out


def _check_family(gpu, family, zr=True, pt=True):
    rows = W.expected(family, zr, pt)
    assert len(rows) == len(W.family(family)) > 0
    be = _block_encoder(gpu, zr, pt)
    try:
        bad = []
        for b, rec, data in rows:
            bad += _diffs(be, b.x, rec, data, f"{family}/{b.name} (n = {b.x.size}, zero runs {zr}, partitions {pt})")
    finally:
        be._enc.close()
    assert not bad, f"{len(bad)} differences:\n" + "\n".join(bad[:40])


@pytest.mark.parametrize("family", W.FAMILIES)
def test_plans_and_bytes_equal_the_oracle(gpu, family):
    _check_family(gpu, family)


@pytest.mark.parametrize("zr,pt", W.FLAGS[1:], ids=["no_partitions", "no_zero_runs", "neither"])
@pytest.mark.parametrize("family", W.FLAG_SUBSET)
def test_other_flag_pairs(gpu, family, zr, pt):
    """The subset that still meets the fallback, partition-geometry and mode conditions under the pair
    (widerecipes.check_flag_coverage)."""
    _check_family(gpu, family, zr, pt)


def test_one_handle_across_sizes_and_paths(gpu, oracle):
    """wide n = 1024 -> narrow n = 300 -> wide n = 13 -> wide n = 16384 -> wide n = 5, twice round, on one handle: the
    residual scratch and the plan slot are reused across sizes and across the two paths; a stale record or a stale tail of
    the scratch shows as a mismatch."""
    blocks = W.sequence_blocks()
    want = [(planref.wide_slot_record(oracle, x), oracle.block_encode(x)) for x in blocks]
    be = _block_encoder(gpu)
    try:
        bad = []
        for lap in range(2):
            for x, (rec, data) in zip(blocks, want):
                bad += _diffs(be, x, rec, data, f"lap {lap}, n = {x.size}")
    finally:
        be._enc.close()
    assert not bad, "\n".join(bad)
