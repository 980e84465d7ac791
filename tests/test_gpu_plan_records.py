"""Every plan record of the device analysis against the oracle: what `lacx_analyze` / `lacx_analyze_device` return, block
record by block record (frames, invalid, est_ms, uncertain, choose_ms), slot by slot (which of the sixteen are valid) and
field by field (predictor type, order, partition order, coefficients, every partition's mode and k, total bits, payload
bytes).  Exact equality everywhere.

The stream tests see one bit per probed block (`ms < lr` over twelve probe sizes): an error common to all probe slots
cancels, one in a single slot hides inside the block's margin (hundreds of bytes).  Here each of the twelve probe records,
both losers of a full comparison, and the estimate's flags are compared on their own.  The expectation and the comparer
are tests/planref.py, the inputs and the conditions they must meet tests/planrecipes.py (both also tested without a GPU,
tests/test_plan_records_host.py).

Predictor type 1 (FIR) wins none of the 9 kinds x 6 stereo families of probe windows; the two extra blocks of case a
(planrecipes.fir_window) are there for it."""
import pytest

import planrecipes as R
import planref

pytestmark = pytest.mark.gpu

BLOCK = planref.BLOCK
RATE = R.RATE


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lacx.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests need an MI355X (the product has no CPU fallback)")
    return pkg


def _encoder(gpu, bits, mode=2, zr=True, pt=True):
    enc = gpu.lacx.Encoder(12, mode, RATE, bits, device=0)
    enc.set_zero_run_enabled(zr)
    enc.set_partitioning_enabled(pt)
    return enc


def _check(enc, expected, left, right, name, block_fields=planref.BLOCK_FIELDS):
    """One analysis on `enc`, every record against the expectation, and the slot counts of lacx_timing."""
    bplans, plans = enc.analyze(left, right)
    planref.assert_same(expected, bplans, plans, name, block_fields)
    t = enc.timing()
    assert (t.full_slots, t.probe_slots) == planref.counts(expected), name


def _analyze(gpu, expected, left, right, bits, name, mode=2, zr=True, pt=True, block_fields=planref.BLOCK_FIELDS):
    enc = _encoder(gpu, bits, mode, zr, pt)
    _check(enc, expected, left, right, name, block_fields)
    enc.close()


@pytest.mark.parametrize("bits", [16, 24])
def test_probe_slots_over_every_kind_of_window(gpu, bits):
    """Case a: 56 blocks, all probed; 56 x 16 slot records (14 valid per block, all fields) and 56 block records."""
    expected = R.expected("a", bits)
    R.check_coverage_a(expected, bits)  # on the oracle's records alone, before the device is touched
    left, right = R.stream_a(bits)
    _analyze(gpu, expected, left, right, bits, f"case a {bits}-bit")


@pytest.mark.parametrize("bits", [16, 24])
def test_halves_of_a_wave_of_different_character(gpu, bits):
    """Case b: 20 blocks (5 patterns x the channel that carries it: L, R, S, M): one slot of a pair is zeros, a constant,
    full-scale alternation, a single +-1, or starts at frame 255, its partner in the wave is noise."""
    expected = R.expected("b", bits)
    R.check_coverage_b(expected)
    left, right = R.stream_b(bits)
    _analyze(gpu, expected, left, right, bits, f"case b {bits}-bit")


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("last", R.FINAL_FRAMES)
def test_final_blocks(gpu, bits, last):
    """Case c: at <= 4096 frames all four whole-block slots are valid and equal the oracle's plans, the two losers
    included, and no probe slot is; above, all twelve probe slots (the middle window starts at an odd frame, an even
    one, a multiple of 64)."""
    expected = R.expected("c", bits, arg=last)
    want_slots = list(range(4)) if last <= planref.FULL_COMPARE_LIMIT else None
    fin = expected[-1]
    assert fin.frames == last and fin.uncertain == 1  # (independent noise: the estimate never settles)
    if want_slots is not None:
        assert sorted(fin.slots) == want_slots
    else:
        assert sorted(s for s in fin.slots if s >= 4) == list(range(4, 16)) and len(fin.slots) == 14
    left, right = R.stream_c(bits, last)
    _analyze(gpu, expected, left, right, bits, f"case c {bits}-bit, final block of {last}")


@pytest.mark.parametrize("bits", [16, 24])
def test_estimate_flags(gpu, bits):
    """Case d, stereo mode 2: est_ms, uncertain, choose_ms, the valid set and every valid record of 231 blocks (the grid of
    8 kinds x 6 families x 4 blocks, the gain sweep, an all-zero block, one silent on the left, one whose only non-zero
    sample is the last)."""
    expected = R.expected("d", bits)
    R.check_coverage_d(expected)
    left, right = R.stream_d(bits)
    _analyze(gpu, expected, left, right, bits, f"case d {bits}-bit")


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("mode", ["left_right", "mid_side", "mono"])
def test_valid_set_without_an_estimate(gpu, bits, mode):
    """Case d in the forced modes and mono: the block record and the valid set of every block (slots 0,1 / 2,3 / 0 and
    nothing else); the records themselves for the first and the last sixteen blocks."""
    left, right = R.stream_d(bits)
    sm = 1 if mode == "mid_side" else 0
    mono = mode == "mono"
    expected = R.expected("d", bits, mode=sm, mono=mono, records=False)
    _analyze(gpu, expected, left, None if mono else right, bits, f"case d {bits}-bit {mode}", mode=sm)
    for sel in (slice(0, 16 * BLOCK), slice(left.size - 16 * BLOCK, left.size)):
        l, r = left[sel], None if mono else right[sel]
        full = tuple(planref.expected_stream(R._oracle(), l, r, sm))
        _analyze(gpu, full, l, r, bits, f"case d {bits}-bit {mode} frames {sel.start}..", mode=sm)


# -- e. the same records whoever produces them --------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("case", ["a", "d"])
def test_records_from_k_stereo_and_k_decide(gpu, monkeypatch, case, bits):
    """LACX_NO_FRONT_FOLD: the block records come from the kernels k_stereo / k_decide instead of the block's last ingest
    workgroup and its last probe slot."""
    monkeypatch.setenv("LACX_NO_FRONT_FOLD", "1")
    left, right = R._STREAMS[case](bits)
    _analyze(gpu, R.expected(case, bits), left, right, bits, f"case {case} {bits}-bit, k_stereo / k_decide")


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("fold", [True, False], ids=["folded", "k_stereo_and_k_decide"])
def test_one_handle_again_and_after_a_stream_without_probes(gpu, monkeypatch, bits, fold):
    """Case a twice in a row on one handle, then a stream with the same number of blocks that are all certain (no probe
    slot, one pair), then case a again, then case d's silent and half-silent tail: a record left valid by the call
    before shows as an extra valid slot, a counter that did not go back to zero as a missing one."""
    if not fold:
        monkeypatch.setenv("LACX_NO_FRONT_FOLD", "1")
    expected = R.expected("a", bits)
    left, right = R.stream_a(bits)
    certain = R.expected("certain", bits, arg=len(expected))
    R.check_coverage_certain(certain)
    cl, cr = R.stream_certain(bits, len(expected))
    enc = _encoder(gpu, bits)
    _check(enc, expected, left, right, f"case a {bits}-bit, first call")
    _check(enc, expected, left, right, f"case a {bits}-bit, second call")
    _check(enc, certain, cl, cr, f"certain stream {bits}-bit after case a")
    _check(enc, expected, left, right, f"case a {bits}-bit after the certain stream")
    dl, dr = R.stream_d(bits)
    tail = slice(dl.size - len(expected) * BLOCK, dl.size)
    _check(enc, R.expected("d", bits)[-len(expected):], dl[tail], dr[tail], f"case d {bits}-bit tail after case a")
    enc.close()


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("case", ["a", "d"])
def test_records_of_device_resident_pcm_on_a_callers_stream(gpu, case, bits):
    """lacx_analyze_device on torch tensors, queued on a stream of the caller's behind the copy that produces them."""
    import torch

    expected = R.expected(case, bits)
    left, right = R._STREAMS[case](bits)
    enc = _encoder(gpu, bits)
    stream = torch.cuda.Stream()
    hl, hr = torch.from_numpy(left).pin_memory(), torch.from_numpy(right).pin_memory()
    with torch.cuda.stream(stream):
        dl, dr = hl.to("cuda", non_blocking=True), hr.to("cuda", non_blocking=True)
        for call in range(2):
            bplans, plans = enc.analyze_device(dl.data_ptr(), dr.data_ptr(), left.size, stream.cuda_stream, plans=True)
            planref.assert_same(expected, bplans, plans, f"case {case} {bits}-bit, device tensors, call {call}")
            t = enc.timing()
            assert (t.full_slots, t.probe_slots) == planref.counts(expected)
    stream.synchronize()
    enc.close()


@pytest.mark.parametrize("zr,pt", [(False, True), (True, False), (False, False)], ids=["no_zero_runs", "no_partitions", "neither"])
@pytest.mark.parametrize("case", ["a", "d"])
def test_records_without_zero_runs_or_partitions(gpu, case, zr, pt):
    bits = 16 if case == "a" else 24
    if case == "d":  # (the whole-block plans are what the oracle is slow at: the sweep and the special blocks, 39 blocks)
        left, right = R.stream_d(bits)
        left, right = left[R.GRID_BLOCKS_D * BLOCK:], right[R.GRID_BLOCKS_D * BLOCK:]
        expected = tuple(planref.expected_stream(R._oracle(), left, right, 2, zr, pt))
    else:
        left, right = R.stream_a(bits)
        expected = R.expected("a", bits, zr=zr, pt=pt)
        assert all(b.uncertain and b.margin is not None for b in expected)
    if not pt:
        assert all(r.partition_order == 0 for b in expected for r in b.slots.values())
    _analyze(gpu, expected, left, right, bits, f"case {case} {bits}-bit zero runs {zr} partitions {pt}", zr=zr, pt=pt)
