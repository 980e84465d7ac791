"""The streaming block kernels (k_analyze<16,1024> with its fused emit and the packer, k_offsets / k_emit / k_pack) against
the oracle over the constructed corpus of tests/narrowrecipes.py: block by block through `BlockEncoder`, as streams record
by record through `Encoder.analyze` and byte by byte through `Encoder.encode` (fused emit, k_emit alone, host emit, the two
repair paths of the hooks library), and every ragged block as a stream of its own in one `BatchEncoder` job.  Exact
equality everywhere, no block left out.  The conditions the corpus meets are asserted on the oracle alone in
tests/test_narrow_blocks_host.py and once more here before the device is asked anything.

Sizes: one stereo stream of 15 + 1 blocks, three single-block stereo streams, 112 single blocks, 74 single-block batch
streams; the oracle's side of the largest test is about 1.5 s.  Per-test GPU wall times: not measured yet."""
import numpy as np
import pytest

import narrowrecipes as N
import planref

pytestmark = pytest.mark.gpu

RATE = 48000


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lacx.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests need an MI355X (the product has no CPU fallback)")
    return pkg


@pytest.fixture(scope="module")
def covered():
    return N.check_coverage()


def _block_encoder(gpu, zr=True, pt=True):
    be = gpu.lacx.BlockEncoder(12)
    be.set_zero_run_enabled(zr)
    be.set_partitioning_enabled(pt)
    return be


def _diffs(be, x, rec, data, what):
    out = [f"{what}: plan {name} = {got}, oracle {want}" for name, got, want in planref.slot_diffs(be.plan(x), rec)]
    got = be.encode(x)
    if got != data:
        first = next((i for i, (a, b) in enumerate(zip(got, data)) if a != b), min(len(got), len(data)))
        out.append(f"{what}: {len(got)} bytes, oracle {len(data)}, first difference at byte {first}")
    return out


def _check_families(gpu, families, zr=True, pt=True):
    """One handle for all the blocks, in corpus order: sizes and characters alternate on one workspace."""
    be = _block_encoder(gpu, zr, pt)
    try:
        bad, count = [], 0
        for family in families:
            for b, rec, data in N.expected(family, zr, pt):
                bad += _diffs(be, b.x, rec, data, f"{family}/{b.name} (n = {b.x.size}, zero runs {zr}, partitions {pt})")
                count += 1
    finally:
        be._enc.close()
    assert count == sum(len(N.family(f)) for f in families)
    assert not bad, f"{len(bad)} differences:\n" + "\n".join(bad[:40])


def test_plans_and_bytes_equal_the_oracle(gpu, covered):
    _check_families(gpu, N.FAMILIES)
    assert sum(covered.values()) == len(N.corpus())


@pytest.mark.parametrize("zr,pt", N.FLAGS[1:], ids=["no_partitions", "no_zero_runs", "neither"])
def test_other_flag_pairs(gpu, zr, pt):
    N.check_flag_coverage()
    _check_families(gpu, N.FLAG_SUBSET, zr, pt)


def _records(gpu, oracle, name, bits, left, right, mode):
    expected = planref.expected_stream(oracle, left, right, mode)
    enc = gpu.lacx.Encoder(12, mode, RATE, bits, device=0)
    try:
        for call in range(2):
            bplans, plans = enc.analyze(left, right)
            planref.assert_same(expected, bplans, plans, f"{name} mode {mode} call {call}")
            t = enc.timing()
            assert (t.full_slots, t.probe_slots) == planref.counts(expected), (name, mode)
    finally:
        enc.close()


@pytest.mark.parametrize("mode", [0, 1], ids=["left_right", "mid_side"])
def test_stream_records(gpu, oracle, covered, mode):
    """Forced left/right and forced mid/side (M and S derived on the fly) over the corpus streams."""
    for name, bits, left, right in N.streams():
        _records(gpu, oracle, name, bits, left, right, mode)


@pytest.mark.parametrize("mode", [1, 2], ids=["mid_side", "per_block"])
def test_stereo_family_records(gpu, oracle, covered, mode):
    """The full-scale pairs: the 25-bit (17-bit) side channel, and the per-block choice with its probes."""
    for name, bits, left, right in N.stereo_streams():
        _records(gpu, oracle, name, bits, left, right, mode)


def _all_streams():
    return [(name, bits, left, right, mode) for name, bits, left, right in N.streams() for mode in (0, 1)] + \
        [(name, bits, left, right, 2) for name, bits, left, right in N.stereo_streams()]


@pytest.mark.parametrize("emit", ["fused", "k_emit_only", "host_emit"])
def test_stream_bytes(gpu, oracle, monkeypatch, emit):
    if emit == "k_emit_only":
        monkeypatch.setenv("LACX_FUSED_EMIT", "0")
    for name, bits, left, right, mode in _all_streams():
        want = oracle.encode(left, right, RATE, bits, mode, threads=8)
        enc = gpu.lacx.Encoder(12, mode, RATE, bits, device=0)
        if emit == "host_emit":
            enc.set_host_emit(True)
        try:
            for call in range(2):
                assert enc.encode(left, right) == want, (name, mode, emit, call)
        finally:
            enc.close()


@pytest.mark.parametrize("hook", ["every_fifth_left_to_k_emit", "packer_gives_up"])
def test_stream_bytes_through_the_repair_paths(gpu, oracle, monkeypatch, request, hook):
    """The hook modes of test_gpu_parity.test_fused_emit_and_its_fallbacks on a corpus stream: k_emit repairs every fifth
    channel block, or the packer gives up and k_pack moves these bitstreams."""
    gpu.lacx.use_library(gpu.lacx.HOOKS_LIB_PATH)
    request.addfinalizer(lambda: gpu.lacx.use_library(None))
    monkeypatch.setenv("LACX_DEBUG_SKIP", "1024" if hook == "every_fifth_left_to_k_emit" else "8192")
    name, bits, left, right = N.streams()[0]
    for mode in (0, 1):
        want = oracle.encode(left, right, RATE, bits, mode, threads=8)
        enc = gpu.lacx.Encoder(12, mode, RATE, bits, device=0)
        try:
            for call in range(2):
                assert enc.encode(left, right) == want, (name, mode, hook, call)
            if hook == "packer_gives_up":
                assert enc.timing().packer_gave_up > 0 and enc.timing().moved_by_k_pack > 0
            else:
                assert 0 < enc.timing().emit_direct < -(-left.size // N.BLOCK) * 2
        finally:
            enc.close()


def _ragged_jobs():
    """[(left, right or None, bit depth, stereo mode, layout)]: every ragged block as a mono stream, and every second pair
    of neighbours of one size as a stereo stream (modes 0, 1, 2 in turn); planar int32 / packed int24 in turn, 16-bit
    material as interleaved int16."""
    blocks = N.ragged_blocks()
    jobs = [(b.x, None) for b in blocks]
    jobs += [(a.x, b.x) for a, b in zip(blocks[0::4], blocks[1::4]) if a.x.size == b.x.size]
    out = []
    for i, (left, right) in enumerate(jobs):
        small = N.fits(left, 16) and (right is None or N.fits(right, 16))
        layout = "i16" if small else ("planar", "i24")[i & 1]
        out.append((left, right, 16 if small else 24, 0 if right is None else i % 3, layout))
    return out


def test_ragged_blocks_as_one_job(gpu, oracle):
    import torch

    jobs = _ragged_jobs()
    assert {j[4] for j in jobs} == {"planar", "i16", "i24"} and sum(1 for j in jobs if j[1] is not None) >= 10
    assert {j[3] for j in jobs if j[1] is not None} == {0, 1, 2}
    keep, streams, want = [], [], []
    for left, right, bits, mode, layout in jobs:
        ch = 1 if right is None else 2
        if layout == "planar":
            dl = torch.from_numpy(np.ascontiguousarray(left)).cuda()
            dr = None if right is None else torch.from_numpy(np.ascontiguousarray(right)).cuda()
            keep += [dl, dr]
            streams.append((dl.data_ptr(), gpu.lacx.PCM_PLANAR_I32, ch, left.size) + (() if dr is None else (dr.data_ptr(),)))
        else:
            inter = gpu.synth.interleave(left, right, bits)
            d = torch.from_numpy(inter.view(np.int16) if bits == 16 else inter).cuda()
            keep.append(d)
            streams.append((d.data_ptr(), gpu.lacx.PCM_INTERLEAVED_I16 if bits == 16 else gpu.lacx.PCM_INTERLEAVED_I24,
                            ch, left.size))
        want.append(oracle.encode(left, right, RATE, bits, mode))
    be = gpu.lacx.BatchEncoder([(RATE, bits, mode) for _, _, bits, mode, _ in jobs], device=0)
    for rep in range(2):
        res = be.encode_device(streams, torch.cuda.current_stream().cuda_stream)
        for i, ((left, right, bits, mode, layout), (pay, tab), w) in enumerate(zip(jobs, res, want)):
            got = gpu.lacx.assemble(RATE, bits, mode, 1 if right is None else 2, [(pay.tobytes(), tab.copy())])
            assert got == w, (i, left.size, bits, mode, layout, rep)
    be._enc.close()
