"""Blocks of 1..4096 samples on the streaming block kernels (k_analyze<16,1024> with its fused emit, k_offsets / k_emit /
k_pack, k_decide phase 2) against the oracle over the constructed corpus of tests/shortrecipes.py:

  a. block by block through one `BlockEncoder` per test (plan fields and bytes), under all four flag pairs, and one handle
     that walks between full and short blocks;
  b. every corpus block as a stream of its own, up to 128 streams per `BatchEncoder` job;
  c. final blocks of per-block stereo, record by record through `Encoder.analyze`: the full comparison of both pairs
     (four whole-block slots, k_decide phase 2, no probes) behind zero, one and two full blocks, in every stereo mode
     and mono, and by the kernels k_stereo / k_decide;
  d. the same streams byte by byte through `Encoder.encode`: fused emit, k_emit alone, host emit, the two repair paths
     of the hooks library.

Exact equality everywhere, no case left out.  The conditions the corpus meets are asserted on the oracle alone in
tests/test_short_blocks_host.py and once more here (check_coverage, cached) before the device is asked anything.

Sizes: 1744 blocks (1639 `lengths` in seven slices, 105 `geometry`), 314 of them under the other three flag pairs; 2135
batch streams (1744 mono, 391 stereo) in 17 jobs; 24 pairs (25 at n = 1, 24 bit) x 3 streams per size and bit depth, at
18 sizes.  `emit_direct` counts the stream indices the packer placed (csrc/api_pipeline.cpp, fused_emit_stats:
h_emitted == 1), so on a fused mode-2 run it is exactly the channel blocks of the full blocks in front: 2 per full
block, none of the final block's (at 4097 frames the final block's two as well).

The reference bytes of a stream with full blocks in front are shortrecipes.stream_bytes: the oracle's encode of the full
blocks spliced with its encode of the final block, held against `oracle.encode(..., threads=8)` of the whole stream for
the first pair and the outcome pairs of every size (final_bytes); encoding each of the 6 900 streams with full blocks
in front whole would cost the oracle 40 ms apiece.

Per-test GPU wall times, measured on an MI355X (589 cases, 230 s together): a `lengths` slice at most 0.25 s (the first
one 1.5 s more for the module's expectation), geometry 0.1 s, a flag pair at most 1.0 s, the one-handle walk 0.2 s, the
batch jobs 0.5 s; records of a size at most 0.5 s, from k_stereo / k_decide 0.03 s; bytes of a size and mode: fused at
most 0.65 s, k_emit alone 0.1 s, host emit 2.2 s (144 encodes); repair paths 0.07 s with every fifth block left to
k_emit and 2.1 s where the packer gives up (96 encodes)."""
import numpy as np
import pytest

import narrowrecipes as N
import planref
import shortrecipes as S

pytestmark = pytest.mark.gpu

RATE = S.RATE
PAIR_SIZES = S.PAIR_N + (S.PAIR_CONTRAST_N,)


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lacx.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests need an MI355X (the product has no CPU fallback)")
    return pkg


@pytest.fixture(scope="module")
def covered():
    return S.check_coverage()


# -- a. blocks, one handle ----------------------------------------------------------------------------------------------

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


def _walk(gpu, rows, zr=True, pt=True):
    """One handle for all the rows, in the order given: sizes and characters alternate on one workspace."""
    be = _block_encoder(gpu, zr, pt)
    try:
        bad = []
        for b, rec, data in rows:
            bad += _diffs(be, b.x, rec, data, f"{b.family}/{b.name} (n = {b.x.size}, zero runs {zr}, partitions {pt})")
    finally:
        be._enc.close()
    assert not bad, f"{len(bad)} differences:\n" + "\n".join(bad[:40])


@pytest.mark.parametrize("sizes", S.LENGTH_SLICES, ids=[f"n{s[0]}_to_{s[-1]}" for s in S.LENGTH_SLICES])
def test_lengths_plans_and_bytes_equal_the_oracle(gpu, covered, sizes):
    rows = S.expected("lengths", True, True, sizes)
    assert len(rows) == len(sizes) * len(S.CHARACTERS)
    _walk(gpu, rows)


def test_geometry_plans_and_bytes_equal_the_oracle(gpu, covered):
    rows = S.expected("geometry")
    assert len(rows) == covered["geometry"] == len(S.family("geometry"))
    _walk(gpu, rows)


@pytest.mark.parametrize("zr,pt", S.FLAGS[1:], ids=["no_partitions", "no_zero_runs", "neither"])
def test_other_flag_pairs(gpu, covered, zr, pt):
    S.check_flag_coverage()
    rows = S.expected_subset(zr, pt)
    assert len(rows) == len(S.flag_subset())
    _walk(gpu, rows, zr, pt)


def test_one_handle_between_full_and_short_blocks(gpu, covered):
    """16384 -> 1 -> 4096 -> 2 -> 16384 -> 65 and back on one handle: a workspace row, a counter or a queue left over
    from a block of 1024 busy threads shows in the block of one thread behind it."""
    o = S.oracle()
    seq = [N.block("geometry", "n16384_p8"), S.block("lengths", "noise24_n1"), S.block("geometry", "n4096_p7"),
           S.block("lengths", "tone_n2"), N.block("tokens", "short_runs_n16384"), S.block("geometry", "n65_p1")]
    assert [b.x.size for b in seq] == [16384, 1, 4096, 2, 16384, 65]
    seq = seq + seq[-2::-1]
    _walk(gpu, [(b, planref.slot_record(o, b.x), o.block_encode(b.x)) for b in seq])


# -- b. every short block as a stream of its own, many per job ----------------------------------------------------------

def _batch_streams():
    """[(left, right or None, bit depth, stereo mode, layout)]: every corpus block as a mono stream (stream_form: inside 24
    bits), and every second pair of neighbours of one size as a stereo stream (modes 0, 1, 2 in turn); planar int32 /
    packed int24 in turn, 16-bit material as interleaved int16."""
    blocks = [S.stream_form(b.x) for b in S.corpus()]
    jobs = [(x, None) for x in blocks]
    jobs += [(a, b) for a, b in zip(blocks[0::4], blocks[1::4]) if a.size == b.size]
    out = []
    for i, (left, right) in enumerate(jobs):
        small = S.fits(left, 16) and (right is None or S.fits(right, 16))
        layout = "i16" if small else ("planar", "i24")[i & 1]
        out.append((left, right, 16 if small else 24, 0 if right is None else i % 3, layout))
    # mono first and stereo last would keep the modes apart: deal the stereo streams in between the mono ones
    mono = [s for s in out if s[1] is None]
    stereo = [s for s in out if s[1] is not None]
    step = len(mono) // len(stereo)
    order = []
    for i, s in enumerate(mono):
        order.append(s)
        if i % step == step - 1 and i // step < len(stereo):
            order.append(stereo[i // step])
    order += stereo[len(mono) // step:]
    assert len(order) == len(out)
    return order


JOB_STREAMS = 128


def test_short_blocks_as_streams_of_batch_jobs(gpu, oracle, covered):
    """Jobs of up to 128 single-block streams of 1, 2, 3, ... frames side by side, each job twice: one workgroup per
    stream, the first_wg search over many streams, 4096-aligned output regions that are almost empty; a mode-2 stereo
    stream here has fuse_items == 0."""
    import torch

    order = _batch_streams()
    assert len(order) >= len(S.corpus()) + 380 and {s[4] for s in order} == {"planar", "i16", "i24"}
    assert {s[3] for s in order if s[1] is not None} == {0, 1, 2}
    assert any(s[3] == 2 and s[0].size == 1 for s in order) and any(s[3] == 2 and s[0].size == 4096 for s in order)
    bad = []
    for a in range(0, len(order), JOB_STREAMS):
        job = order[a:a + JOB_STREAMS]
        keep, args, want = [], [], []
        for left, right, bits, mode, layout in job:
            ch = 1 if right is None else 2
            if layout == "planar":
                dl = torch.from_numpy(np.ascontiguousarray(left)).cuda()
                dr = None if right is None else torch.from_numpy(np.ascontiguousarray(right)).cuda()
                keep += [dl, dr]
                args.append((dl.data_ptr(), gpu.lacx.PCM_PLANAR_I32, ch, left.size) + (() if dr is None else (dr.data_ptr(),)))
            else:
                inter = gpu.synth.interleave(left, right, bits)
                d = torch.from_numpy(inter.view(np.int16) if bits == 16 else inter).cuda()
                keep.append(d)
                args.append((d.data_ptr(), gpu.lacx.PCM_INTERLEAVED_I16 if bits == 16 else gpu.lacx.PCM_INTERLEAVED_I24,
                             ch, left.size))
            want.append(oracle.encode(left, right, RATE, bits, mode))
        be = gpu.lacx.BatchEncoder([(RATE, bits, mode) for _, _, bits, mode, _ in job], device=0)
        try:
            for rep in range(2):
                res = be.encode_device(args, torch.cuda.current_stream().cuda_stream)
                for i, ((left, right, bits, mode, layout), (pay, tab), w) in enumerate(zip(job, res, want)):
                    got = gpu.lacx.assemble(RATE, bits, mode, 1 if right is None else 2, [(pay.tobytes(), tab.copy())])
                    if got != w:
                        bad.append(f"job {a // JOB_STREAMS} stream {i}: {left.size} frames, {bits} bit, "
                                   f"{'mono' if right is None else f'stereo mode {mode}'}, {layout}, run {rep}: "
                                   f"{len(got)} bytes, oracle {len(w)}")
        finally:
            be._enc.close()
    assert not bad, f"{len(bad)} differences:\n" + "\n".join(bad[:40])


# -- c. final blocks, records -------------------------------------------------------------------------------------------

def _encoder(gpu, bits, mode):
    return gpu.lacx.Encoder(12, 0 if mode == "mono" else mode, RATE, bits, device=0)


def _records(gpu, bits, n, mode, only=None):
    """Every stream of the size twice in a row on one handle that walks them all."""
    streams, expected = S.final_streams(bits, n), S.expected_final(bits, n, mode)
    enc = _encoder(gpu, bits, mode)
    count = 0
    try:
        for j, ((name, k, left, right), exp) in enumerate(zip(streams, expected)):
            if only is not None and j // len(S.FRONTS) not in only:
                continue
            for call in range(2):
                bplans, plans = enc.analyze(left, None if mode == "mono" else right)
                planref.assert_same(exp, bplans, plans, f"{name} mode {mode} call {call}")
                t = enc.timing()
                assert (t.full_slots, t.probe_slots) == planref.counts(exp), (name, mode, call)
            count += 1
    finally:
        enc.close()
    return count


def _check_expectation(bits, n):
    """The form of the mode-2 expectation, on the oracle alone: a short final block that is not decided by the estimate
    has exactly the four whole-block slots, both losers included; at 4097 frames the twelve probe slots instead."""
    seen = set()
    for (name, k, left, right), exp in zip(S.final_streams(bits, n), S.expected_final(bits, n, 2)):
        fin = exp[-1]
        assert len(exp) == k + 1 and fin.frames == n
        if not fin.uncertain:
            assert sorted(fin.slots) == ([2, 3] if fin.est_ms else [0, 1]) and fin.choose_ms == fin.est_ms, name
        elif n <= S.LIMIT:
            assert sorted(fin.slots) == [0, 1, 2, 3], name
            assert fin.choose_ms == int(fin.slots[2].payload_bytes + fin.slots[3].payload_bytes <
                                        fin.slots[0].payload_bytes + fin.slots[1].payload_bytes), name
        elif left[-n:].any() or right[-n:].any():
            assert sorted(fin.slots)[2:] == list(range(4, 16)) and len(fin.slots) == 14, name
        seen.add((bool(fin.uncertain), len(fin.slots)))
    assert (True, 4 if n <= S.LIMIT else 14) in seen, (bits, n, seen)


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("n", PAIR_SIZES)
def test_final_block_records(gpu, covered, bits, n):
    """Per-block stereo, forced left/right, forced mid/side and mono over every pair of the size behind 0, 1 and 2 full
    blocks."""
    _check_expectation(bits, n)
    for mode in S.STREAM_MODES:
        assert _records(gpu, bits, n, mode) == len(S.pairs(bits, n)) * len(S.FRONTS)


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("n", PAIR_SIZES)
def test_final_block_records_from_k_stereo_and_k_decide(gpu, covered, monkeypatch, bits, n):
    """LACX_NO_FRONT_FOLD: k_stereo and k_decide run as kernels; the first pair of each outcome the size reaches (at 4097:
    the first eight pairs)."""
    monkeypatch.setenv("LACX_NO_FRONT_FOLD", "1")
    only = S.outcome_pairs(bits, n) if n <= S.LIMIT else tuple(range(8))
    assert _records(gpu, bits, n, 2, only) == len(only) * len(S.FRONTS)


# -- d. final blocks, bytes ---------------------------------------------------------------------------------------------

def _bytes(gpu, bits, n, mode, emit, fronts=S.FRONTS):
    streams, want = S.final_streams(bits, n), S.final_bytes(bits, n, mode)
    enc = _encoder(gpu, bits, mode)
    if emit == "host_emit":
        enc.set_host_emit(True)
    count = 0
    try:
        for (name, k, left, right), w in zip(streams, want):
            if k not in fronts:
                continue
            for call in range(2):
                assert enc.encode(left, None if mode == "mono" else right) == w, (name, mode, emit, call)
                if emit == "fused" and mode == 2 and k and n <= S.LIMIT:
                    assert enc.timing().emit_direct == 2 * k, (name, call, enc.timing().emit_direct)
            count += 1
    finally:
        enc.close()
    return count


@pytest.mark.parametrize("emit", ["fused", "k_emit_only", "host_emit"])
@pytest.mark.parametrize("mode", S.STREAM_MODES, ids=["left_right", "mid_side", "per_block", "mono"])
@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("n", PAIR_SIZES)
def test_final_block_bytes(gpu, covered, monkeypatch, bits, n, mode, emit):
    """The streams of test_final_block_records through `Encoder.encode`, twice per handle: in per-block stereo a call over
    a stream with full blocks in front mixes fused slots with slots that only k_emit writes, and a stream that is only
    the final block has no packer at all."""
    if emit == "k_emit_only":
        monkeypatch.setenv("LACX_FUSED_EMIT", "0")
    assert _bytes(gpu, bits, n, mode, emit) == len(S.pairs(bits, n)) * len(S.FRONTS)


@pytest.mark.parametrize("hook", ["every_fifth_left_to_k_emit", "packer_gives_up"])
@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("n", PAIR_SIZES)
def test_final_block_bytes_through_the_repair_paths(gpu, covered, monkeypatch, request, bits, n, hook):
    """The hook modes of test_gpu_narrow_blocks.test_stream_bytes_through_the_repair_paths on the streams with two full
    blocks in front, in per-block stereo (where the final block is outside the fused emit) and forced left/right (where
    it is inside); forced mid/side and mono go through the repair paths in test_gpu_narrow_blocks and test_gpu_parity."""
    gpu.lacx.use_library(gpu.lacx.HOOKS_LIB_PATH)
    request.addfinalizer(lambda: gpu.lacx.use_library(None))
    monkeypatch.setenv("LACX_DEBUG_SKIP", "1024" if hook == "every_fifth_left_to_k_emit" else "8192")
    for mode in (2, 0):
        assert _bytes(gpu, bits, n, mode, hook, fronts=(2,)) == len(S.pairs(bits, n))
