"""k_ingest and k_stereo on the device, launched as the product launches them over caller-placed PCM (csrc/k_front_hooks.hip,
in liblacx_hooks.so only): every word of sums, badidx, acorr, the block plans and the two need masks against the exact
integers of tests/ingestrecipes.py, the sentinel wherever nothing may be written, front_ctr zero after every run.  No
tolerance anywhere."""
import numpy as np
import pytest

import ingestdev
import ingestrecipes as R

pytestmark = pytest.mark.gpu

FOLDS = pytest.mark.parametrize("fold", (1, 0), ids=("folded", "k_stereo"))


@pytest.fixture(scope="module")
def dev(pkg):
    if pkg.lacx.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests need an MI355X (the product has no CPU fallback)")
    pkg.lacx.use_library(pkg.lacx.HOOKS_LIB_PATH)
    d = None
    try:
        d = ingestdev.Device(pkg.lacx)
        yield d
    finally:
        if d is not None:
            d.close()
        pkg.lacx.use_library(None)


@pytest.fixture(scope="module")
def want(oracle):
    """The reference, computed once and left unchanged: name -> Tables of every corpus stream."""
    return {name: R.expected(st, oracle) for name, st in R.corpus().items()}


def _groups():
    """The corpus in four parts of similar weight (a test function stays at seconds)."""
    names = list(R.corpus())
    big = [n for n in names if R.corpus()[n].blocks >= 7]
    small = [n for n in names if n not in big]
    return {"lengths": [n for n in small if n.startswith("len")], "cases": [n for n in small if not n.startswith("len")],
            "sets-7-8-9": [n for n in big if R.corpus()[n].blocks <= 9], "sets-17-33": [n for n in big if R.corpus()[n].blocks > 9]}


@FOLDS
@pytest.mark.parametrize("group", list(_groups()))
def test_one_stream_sets_equal_the_reference(dev, want, group, fold):
    """Every corpus stream as a launch set of its own, the descriptor in the kernel arguments and in a one-row table."""
    names = _groups()[group]
    assert names
    for name in names:
        p = dev.place(R.corpus()[name])
        for as_table in (False, True):
            runs, ctr = dev.run([p], as_table, fold)
            ingestdev.check(want[name], runs, ctr, f"{name} ({'table' if as_table else 'single'}, fold {fold})")
        assert p.untouched(), name


@FOLDS
@pytest.mark.parametrize("table", [ls.name for ls in R.tables()])
def test_stream_tables_equal_the_reference(dev, want, table, fold):
    """Several streams in one launch set -- mono, LR, MS and per-block stereo, both depths, 23 / 14 / 9 blocks -- twice on
    the same workspace: the second run's bytes are the first's, front_ctr is zero after each."""
    ls = next(x for x in R.tables() if x.name == table)
    placed = [dev.place(s) for s in ls.streams]
    runs, ctr = dev.run(placed, True, fold, repeat=2)
    ingestdev.check(R.concat([want[s.name] for s in ls.streams]), runs, ctr, f"table {table} (fold {fold})")
    assert all(p.untouched() for p in placed)


@FOLDS
def test_repeated_runs_leave_the_counters_zero(dev, want, fold):
    """repeat = 3 without re-zeroing front_ctr, one-stream sets: per-block stereo, and the streams of which only some of
    the four workgroups of a block do work -- mono (one), forced LR / MS (two; with validation four) -- the others only
    count."""
    for name in ("s37768", "s16385", "s33068", "s33068ms", "bad_ms16", "const_fs16", "wide_i24_d24", "b9", "zero_big"):
        p = dev.place(R.corpus()[name])
        runs, ctr = dev.run([p], False, fold, repeat=3)
        assert len(runs) == 3
        ingestdev.check(want[name], runs, ctr, f"{name} x3 (fold {fold})")


@FOLDS
@pytest.mark.parametrize("name", ("lay2", "lay1"))
def test_layouts_and_offsets_give_identical_tables(dev, want, name, fold):
    """The same content as planar int32, interleaved int16 and packed int24, 16-byte aligned (the span fetch) and 4, 8, 12
    -- int24 also 1, 2, 3 -- bytes off (the per-sample path), and at the very end of an allocation: the reference's
    words, the same bytes in every variant, the guard sentinels untouched."""
    first = None
    for v in R.layout_variants(name):
        p = dev.place(v)
        runs, ctr = dev.run([p], False, fold)
        ingestdev.check(want[name], runs, ctr, f"{v.name} (fold {fold})")
        assert p.untouched(), f"{v.name}: a guard byte or the PCM itself was written"
        first = first or runs[0]
        for f in ("sums", "badidx", "acorr", "bplans", "need_probe", "need_full"):
            assert getattr(runs[0], f).tobytes() == getattr(first, f).tobytes(), (v.name, f)


@FOLDS
def test_device_words_refute_every_named_fault(dev, want, fold):
    """The comparison is sharp on the device too: for each mistake the reference can be told to make, the device's words
    of the stream that sees it equal the true reference and differ from the mistaken one."""
    for fault, (text, names) in R.FAULTS.items():
        st = R.corpus()[names[0]]
        runs, ctr = dev.run([dev.place(st)], False, fold)
        ingestdev.check(want[st.name], runs, ctr, f"{st.name} (fold {fold})")
        assert R.differences(R.expect_stream(st, faults={fault}), runs[0], st.name), f"{fault} ({text}) would pass on {st.name}"


def test_hook_refuses_bad_arguments(dev):
    """Host-side validation: LACX_E_INVALID with a message, nothing launched."""
    lx = dev.lacx
    p = dev.place(R.corpus()["len17"])
    good = p.record()

    def bad(**kw):
        rec = ingestdev.HookIngestStream(*[getattr(good, f) for f, _ in good._fields_])
        for k, v in kw.items():
            setattr(rec, k, v)
        return rec

    for rec, blocks, repeat, text in ((bad(frames=0), 1, 1, "stream shape"), (bad(channels=3), 1, 1, "stream shape"),
                                      (bad(stereo_mode=3), 1, 1, "stream shape"), (bad(bit_depth=20), 1, 1, "bit depth"),
                                      (bad(layout=3), 1, 1, "layout"), (bad(layout=R.I16, bit_depth=24, data1=None), 1, 1, "16-bit containers"),
                                      (bad(data1=None), 1, 1, "do not fit"), (bad(data0=good.data0 + 2), 1, 1, "4-byte aligned"),
                                      (good, 2, 1, "not total_blocks"), (good, 1, 0, "repeat"), (good, 1, 17, "repeat")):
        rc, msg, t, _ = _call(dev, rec, blocks, repeat)
        assert rc == lx.E_INVALID and text in msg, (rc, msg, text)
        assert not R.differences(R.sentinel_tables(blocks), R.Tables(t.sums[0], t.badidx[0], t.acorr[0], t.bplans[0], t.need_probe[0], t.need_full[0]), "refused")
    assert p.untouched()


def _call(dev, rec, blocks, repeat):
    """dev.call with buffers for at least one run, whatever `repeat` is handed to the hook."""
    import ctypes as C

    t = R.sentinel_tables(blocks, 1)
    ctr = np.zeros((1, blocks, 2), dtype=np.uint32)
    fn = dev.lacx.lib().lacx_hook_ingest_tables
    fn.restype = C.c_int
    arr = (ingestdev.HookIngestStream * 1)(rec)
    rc = fn(dev.h, arr, C.c_uint32(1), C.c_int(0), C.c_int(1), C.c_uint32(repeat), C.c_uint32(blocks), ingestdev._p(t.sums),
            ingestdev._p(t.badidx), ingestdev._p(t.acorr), ingestdev._p(t.bplans), ingestdev._p(t.need_probe),
            ingestdev._p(t.need_full), ingestdev._p(ctr))
    return rc, dev.lacx.lib().lacx_last_error(dev.h).decode(errors="replace"), t, ctr


def test_slot_0_is_what_the_product_reads_back(dev, want, pkg):
    """The tie to the product: BlockEncoder.debug_lpc on liblacx.so -- a one-block mono launch of the same kernel through
    the encoder's own workspace -- returns the 13 words of the hook's slot 0 for corpus blocks of every length class."""
    lx = pkg.lacx
    picks = [("len17", 0), ("len257", 0), ("len4097", 1), ("len8193", 0), ("s37768", 1), ("impulses", 0), ("big_sums", 1)]
    hook = {}
    for name, ch in picks:
        st = R.corpus()[name]
        x = np.ascontiguousarray((st.left, st.right)[ch][:R.BLOCK])
        mono = R.Stream(f"{name}.{ch}", x, None, 0, 0)
        runs, ctr = dev.run([dev.place(mono)], False, 1)
        assert not ctr.any()
        assert np.array_equal(runs[0].acorr[0, 0], want[name].acorr[0, ch]), name
        hook[name] = (x, runs[0].acorr[0, 0].copy())
    lx.use_library(None)
    try:
        be = lx.BlockEncoder(12, device=0)
        for name, (x, words) in hook.items():
            ac, _, _ = be.debug_lpc(x)
            assert np.array_equal(ac, words), f"{name}: lacx_debug_lpc {ac.tolist()} != hook slot 0 {words.tolist()}"
        be._enc.close()
    finally:
        lx.use_library(lx.HOOKS_LIB_PATH)
