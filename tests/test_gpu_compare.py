"""Bit-compare on the MI355X: lacx_decoder_compare_batch_device, lacx_decoder_compare_pcm_batch_device,
lacx_decoder_item_compare_rows / _compare_counts and `lacx_cli compare`.  The device's counts, rows and totals are held to the
plain CPU twin's (tests/native/sim_compare.cpp) and to the numpy restatement (tests/comparetwin.py) BYTE FOR BYTE: everything
is an exact integer that does not depend on the order of evaluation, there is no tolerance.  Only shapes the sanitized twin has
passed in this run go to the device."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import comparetwin as ct
import lacmutate

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "lossless-audio-codec_amd")


@pytest.fixture(scope="module")
def gpu():
    pkg = ge.load_pkg()
    if pkg.lacx.device_count() <= 0:
        pytest.fail("no HIP device: the decoder has no CPU fallback")
    return pkg


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def as_twin(r):
    """A CompareResult of the binding as the twin's record, so that one check serves both."""
    totals = np.frombuffer(bytes(r.totals), ct.TOTAL_T)[0]
    rows = np.frombuffer(b"".join(bytes(x) for x in r.rows), ct.ROW_T) if r.rows else np.zeros(0, ct.ROW_T)
    return ct.TwinPair(0, "", totals, rows, np.asarray(r.counts, np.uint64))


def same_as_twin(got, twin, what):
    assert got.counts.tobytes() == twin.counts.tobytes() and got.rows.tobytes() == twin.rows.tobytes() and got.totals.tobytes() == twin.totals.tobytes(), what


@pytest.fixture(scope="module")
def twins():
    """{pair name: TwinPair of the plain twin}, every corpus pair, once the sanitized twin has passed them as source jobs."""
    small = ct.small_corpus()
    big = [p for p in ct.corpus() if p.name == "r32767"]
    cases = [ct.source_case(*ct.job(small)), ct.source_case(*ct.job(big))]
    ct.cleared("gpu-corpus", cases)  # CPU first
    out = dict(zip((p.name for p in small), ct.run(cases[0])))
    (out["r32767"],) = ct.run(cases[1])
    return out


@pytest.fixture(scope="module")
def streams(oracle, twins):
    """{pair name: its one or two streams}: the whole corpus."""
    return {p.name: ct.encode(oracle, ct.job([p])[0]) for p in ct.corpus()}


def stream_job(ps, lacs_by):
    lacs, recs = [], []
    for p in ps:
        mine = lacs_by[p.name]
        recs.append((len(lacs), len(lacs) + len(mine) - 1, p.centre, p.radius))
        lacs += mine
    return lacs, recs


@pytest.mark.parametrize("reverse", [False, True])
def test_the_corpus_in_one_batch(gpu, streams, twins, reverse):
    """One stream-form batch of the whole corpus, forward and reversed: pairs, their streams, tiles and rows start at other
    places of the job."""
    ps = ct.corpus()[::-1] if reverse else ct.corpus()
    lacs, recs = stream_job(ps, streams)
    dec = gpu.lacx.Decoder(device=0)
    got = dec.compare_batch(lacs, recs)
    assert dec.last_ms > 0
    for p, g in zip(ps, got):
        ct.check(p, as_twin(g), "device")
        same_as_twin(as_twin(g), twins[p.name], p.name)
        assert len(g.offsets) == (2 * p.radius + 1 if p.radius else 0)
    p = ps[3]
    one = dec.compare(*streams[p.name][:1], streams[p.name][-1], p.centre, p.radius)
    same_as_twin(as_twin(one), twins[p.name], "alone")
    t = one.totals
    if t.mismatches:
        assert t.peak_dbfs <= 20 * np.log10(2.0) + 1e-9 and t.rms_dbfs <= t.peak_dbfs + 1e-9
    dec.close()


def _arrays(x, layout, depth):
    """A source's arrays as bytes: one for an interleaved layout, one per channel for a planar one."""
    chans = [np.asarray(c, np.int32) for c in x]
    if layout in (ct.PF32, ct.IF32):
        chans = [(c.astype(np.float32) / np.float32(1 << (depth - 1))) for c in chans]
    elif layout in (ct.I16, ct.P16):
        chans = [c.astype("<i2") for c in chans]
    if layout == ct.I24:
        inter = np.stack(chans, axis=1).astype("<i4")
        return [inter.view(np.uint8).reshape(-1, 4)[:, :3].tobytes()]
    if layout in (ct.I16, ct.IF32):
        return [np.stack(chans, axis=1).tobytes()]
    return [c.tobytes() for c in chans]


def _upload(torch, raw: bytes, offset=0):
    """raw at `offset` bytes behind the start of a device buffer that ends with it."""
    buf = torch.zeros(offset + len(raw), dtype=torch.uint8, device="cuda")
    buf[offset:] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    return buf


def _device_sources(torch, sources, layout, offset, keep):
    out = []
    for x, depth, rate in sources:
        lay = ct.layout_for(layout, depth)
        off = offset if lay == layout else (offset + 3) // 4 * 4
        bufs = [_upload(torch, raw, off) for raw in _arrays(x, lay, depth)]
        keep.append(bufs)
        ptrs = [b.data_ptr() + off for b in bufs]
        out.append(((ptrs[0], ptrs[1] if len(ptrs) == 2 else None, lay, x.shape[0], x.shape[1]), rate, depth))
    return out


LAYOUT_PAIRS = ("shift|3|diffs", "shift|-2|diffs", "shift|-1", "shift|2", "len|7", "len|4097", "len|9|longer-a", "mono24|row2", "range|24|2", "range|16|1", "radius|300")
LAYOUTS = ((ct.P32, 4), (ct.P32, 12), (ct.I16, 4), (ct.I24, 1), (ct.I24, 6), (ct.P16, 2), (ct.P16, 6), (ct.PF32, 4), (ct.IF32, 8))


def test_source_form_in_every_layout(gpu, torch, twins):
    """Device-resident PCM in every layout that holds the depth, at a nonzero byte offset in buffers that end with the
    source's last byte: the answers are the twin's byte for byte, whatever the layout."""
    by = {p.name: p for p in ct.corpus()}
    ps = [by[n] for n in LAYOUT_PAIRS]
    src, recs = ct.job(ps)
    ct.cleared("gpu-layouts", [ct.source_case(src, recs, layout, off) for layout, off in LAYOUTS])  # CPU first
    dec = gpu.lacx.Decoder(device=0)
    for layout, off in LAYOUTS:
        keep = []
        got = dec.compare_pcm_batch(_device_sources(torch, src, layout, off, keep), recs)
        assert dec.last_ms > 0
        for p, g in zip(ps, got):
            ct.check(p, as_twin(g), (layout, off))
            same_as_twin(as_twin(g), twins[p.name], (p.name, layout, off))
    dec.close()


def test_one_source_in_many_pairs(gpu, torch, twins):
    by = {p.name: p for p in ct.corpus()}
    x = by["shift|3"]
    src = [(x.a, x.depth, x.rate), (x.b, x.depth, x.rate), (by["shift|3|diffs"].b, x.depth, x.rate)]
    recs = [(0, 1, 0, 8), (0, 2, 0, 8), (1, 0, 0, 8), (0, 0, 2, 1), (2, 1, 0, 0)]
    ct.cleared("gpu-many", [ct.source_case(src, recs)])  # CPU first
    twin = ct.run(ct.source_case(src, recs))
    dec = gpu.lacx.Decoder(device=0)
    keep = []
    got = dec.compare_pcm_batch(_device_sources(torch, src, ct.P32, 0, keep), recs)
    for (a, b, c, r), g, t in zip(recs, got, twin):
        ct.check(ct.Pair("many|%d|%d" % (a, b), src[a][0], src[b][0], c, r, x.depth, x.rate), as_twin(g))
        same_as_twin(as_twin(g), t, (a, b))
    assert got[0].offset == 3 and got[2].offset == -3 and got[3].mismatches > 0 and got[0].identical
    dec.close()


def _broken(lac):
    """The stream with one byte of its second block's payload changed: that block does not decode."""
    ent, pays = lacmutate._payloads(lac)
    pays[1] = pays[1][:1] + bytes([0x7F]) + pays[1][2:] if lac[4] == 2 else bytes([0x7F]) + pays[1][1:]
    return lacmutate._rebuild(lac, ent, pays)


def test_a_damaged_stream_fails_its_pairs_alone(gpu, oracle, twins):
    """The middle stream of three does not decode: the pairs that name it keep the decode's code and text behind "source 1: "
    and get no answer; the other pairs are unaffected."""
    xs = [ct.noise(17000, 2, 16, 9000), ct.noise(17000, 2, 16, 9001)]
    xs.append(ct.plant(ct.shifted(xs[0], 2), [(1, 9000)], 9002))
    lacs = ct.encode(oracle, [(x, 16, 44100) for x in xs])
    lacs[1] = _broken(lacs[1])
    recs = [(0, 2, 0, 4), (0, 1, 0, 4), (1, 1, 0, 0), (2, 0, -1, 3)]
    ct.cleared("gpu-damaged", [ct.stream_case(lacs, recs)])  # CPU first
    twin = ct.run(ct.stream_case(lacs, recs))
    assert twin[1].code == 2 and twin[2].code == 2 and not twin[0].code and not twin[3].code
    lx = gpu.lacx
    dec = lx.Decoder(device=0)
    with pytest.raises(lx.BatchDecodeError) as e:
        dec.compare_batch(lacs, recs)
    with pytest.raises(lx.BatchDecodeError) as g:
        dec.digest_batch([lacs[1]])
    assert sorted(e.value.errors) == [1, 2] and e.value.errors[1] == e.value.errors[2] == "source 1: " + g.value.errors[0]
    assert g.value.errors[0].startswith("[decode-error] block=1 ") and e.value.results[1] is None and str(e.value).startswith("pair 1: source 1: [decode-error]")
    with pytest.raises(lx.BatchDecodeError):
        dec.compare_batch(lacs, recs)
    ptr, count = lx.C.POINTER(lx.CompareRow)(), lx.C.c_uint32(5)
    assert lx.lib().lacx_decoder_item_compare_rows(dec._h, 1, lx.C.byref(ptr), lx.C.byref(count)) == lx.E_INVALID and count.value == 0
    for k in (0, 3):
        same_as_twin(as_twin(e.value.results[k]), twin[k], k)
    with pytest.raises(RuntimeError, match="source 1: .decode-error. block=1 "):
        dec.compare(lacs[0], lacs[1])
    dec.close()


def test_an_invalid_float_sample_fails_its_pairs(gpu, torch, twins):
    """An inexact float and a planar int32 outside the depth: the digest form's text behind "source k: ", no answer, the other
    pairs unharmed."""
    by = {p.name: p for p in ct.corpus()}
    ps = [by["shift|1"], by["shift|-1|diffs"], by["identical"]]
    src, recs = ct.job(ps)
    bads = ((ct.PF32, (3, 5000, 0, 0x3E99999A), "source 3: left sample at index 5000 is not an exact 16-bit PCM value"),
            (ct.P32, (2, 17, 0, 0x01000000), "source 2: left sample at index 17 is outside the configured PCM bit depth"))
    ct.cleared("gpu-invalid", [ct.source_case(src, recs, layout, 0, bad) for layout, bad, _ in bads])  # CPU first
    dec = gpu.lacx.Decoder(device=0)
    for layout, (i, frame, ch, word), text in bads:
        keep = []
        dsrc = _device_sources(torch, src, layout, 0, keep)
        assert dsrc[i][0][2] == layout
        keep[i][ch].view(torch.int32)[frame] = word - (1 << 32) if word >= 1 << 31 else word
        with pytest.raises(gpu.lacx.BatchDecodeError) as e:
            dec.compare_pcm_batch(dsrc, recs)
        assert e.value.errors == {1: text} and e.value.codes == {1: gpu.lacx.E_INVALID} and e.value.results[1] is None
        for q in (0, 2):
            same_as_twin(as_twin(e.value.results[q]), twins[ps[q].name], q)
    dec.close()


def test_the_refusals(gpu, torch, twins):
    """Every refusal with its text, each failing its pair on the host; the pair beside them runs."""
    lx = gpu.lacx
    by = {p.name: p for p in ct.corpus()}
    good = by["shift|-2"]  # stereo 24 bit 96000
    src = [(good.a, 24, 96000), (good.b, 24, 96000), (good.a[:1], 24, 96000), (by["shift|1"].a, 16, 96000), (good.a, 24, 48000)]
    assert good.a.shape[0] == 2 and good.depth == 24 and by["shift|1"].a.shape[0] == 1
    keep = []
    dsrc = _device_sources(torch, src, ct.P32, 0, keep)
    mono16 = dsrc[3]
    dsrc[3] = ((mono16[0][0], mono16[0][0], ct.P32, 2, mono16[0][4]), 96000, 16)  # two channels of 16 bit
    recs = [(0, 1, 0, 4), (0, 5, 0, 0), (0, 2, 0, 0), (0, 3, 0, 0), (0, 4, 0, 0), (0, 1, 0, 32768), (0, 1, 2 ** 31 - 4, 4), (0, 1, -2 ** 31, 0), (1, 0, 0, 32767)]
    dec = lx.Decoder(device=0)
    with pytest.raises(lx.BatchDecodeError) as e:
        dec.compare_pcm_batch(dsrc, recs)
    assert e.value.errors == {1: "sources outside the call's array", 2: "channel counts differ (2, 1)", 3: "bit depths differ (24, 16)",
                              4: "sample rates differ (96000, 48000)", 5: "radius above 32767", 6: "centre out of range", 7: "centre out of range"}
    assert all(c == lx.E_INVALID for c in e.value.codes.values())
    same_as_twin(as_twin(e.value.results[0]), ct.run(ct.source_case(src[:2], [(0, 1, 0, 4)]))[0], "beside the refused")
    assert e.value.results[8].offset == 2 and e.value.results[0].offset == -2
    bad = list(dsrc)
    bad[1] = ((dsrc[1][0][0], dsrc[1][0][1], ct.P32, 2, 0), 96000, 24)
    with pytest.raises(lx.BatchDecodeError) as e:
        dec.compare_pcm_batch(bad, [(0, 1, 0, 0), (0, 0, 0, 0)])
    assert e.value.errors == {0: "source 1: source has no frames"} and e.value.results[1].identical
    lacs = [lx.Encoder(12, 2, 44100, 16, device=0).encode(*ct.noise(3000, 2, 16, 1)), lx.Encoder(12, 2, 48000, 16, device=0).encode(*ct.noise(3000, 2, 16, 2)), b"XXXX" + bytes(64)]
    with pytest.raises(ValueError, match=r"sample rates differ \(44100, 48000\)"):
        dec.compare(lacs[0], lacs[1])
    with pytest.raises(lx.BatchDecodeError) as e:
        dec.compare_batch(lacs, [(0, 2, 0, 0), (0, 0, 0, 1)])
    assert e.value.errors[0].startswith("source 2: ") and e.value.codes[0] != lx.OK and e.value.results[1].identical
    dec.close()


def test_radius_0_is_one_round_trip(gpu, streams, twins):
    """A job whose pairs all have radius 0 launches no search: no pair has counts, the counts call gives none, and the answer is
    the rows' at the centre.  A pair of radius 0 beside a searched one has none either."""
    lx = gpu.lacx
    ps = [p for p in ct.corpus() if p.radius == 0][:6]
    assert len(ps) == 6
    lacs, recs = stream_job(ps, streams)
    dec = lx.Decoder(device=0)
    got = dec.compare_batch(lacs, recs)
    for k, (p, g) in enumerate(zip(ps, got)):
        same_as_twin(as_twin(g), twins[p.name], p.name)
        ptr, count = lx.C.POINTER(lx.C.c_uint64)(), lx.C.c_uint32(5)
        assert lx.lib().lacx_decoder_item_compare_counts(dec._h, k, lx.C.byref(ptr), lx.C.byref(count)) == lx.OK and count.value == 0 and not ptr
        assert g.offset == p.centre
    searched = next(p for p in ct.corpus() if p.radius == 8)
    lacs, recs = stream_job([ps[0], searched], streams)
    got = dec.compare_batch(lacs, recs)
    assert len(got[0].counts) == 0 and len(got[1].counts) == 17
    same_as_twin(as_twin(got[0]), twins[ps[0].name], "beside a search")
    dec.close()


def _cli():
    subprocess.check_call(["make", "-C", PKG_DIR, "lacx_cli"], stdout=subprocess.DEVNULL)
    return os.path.join(PKG_DIR, "lacx_cli")


def test_cli_finds_a_planted_offset(gpu, streams, twins, tmp_path):
    """`lacx_cli compare` between a .lac and a WAV: the planted offset, and exit 0 (identical at the chosen offset), 1 (they
    differ) and 2 (refused)."""
    cli = _cli()
    by = {p.name: p for p in ct.corpus()}
    clean, diffs = by["shift|3"], by["shift|3|diffs"]
    assert clean.a.shape[0] == 1 and clean.depth == 16
    dec = gpu.lacx.Decoder(device=0)
    files = {"a.lac": streams[clean.name][0], "b.wav": dec.decode_wav(streams[clean.name][1]), "c.wav": dec.decode_wav(streams[diffs.name][1]),
             "c.lac": streams[diffs.name][1], "d.lac": streams["shift|-1"][0]}
    dec.close()
    for name, blob in files.items():
        with open(str(tmp_path / name), "wb") as f:
            f.write(blob)
    path = lambda n: str(tmp_path / n)  # noqa: E731
    res = subprocess.run([cli, "compare", path("a.lac"), path("b.wav"), "--radius=300"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stderr == "", res.stderr
    assert res.stdout.splitlines()[0].startswith("offset=3 identical") and "lead=3 (B)" in res.stdout
    want = ct.expected(diffs).totals
    for b in ("c.wav", "c.lac"):
        res = subprocess.run([cli, "compare", path("a.lac"), path(b), "--radius=300", "--offsets", "--blocks"], capture_output=True, text=True, timeout=120)
        assert res.returncode == 1 and res.stderr == "", res.stderr
        lines = res.stdout.splitlines()
        assert lines[0].startswith("offset=3 mismatches=%d (%d)" % (int(want["mismatches"]), int(want["ch"][0]["mismatches"]))), lines[0]
        assert "peak=%d" % int(want["peak"]) in lines[0] and sum(1 for t in lines if t.startswith("o=")) == 601 and sum(1 for t in lines if t.startswith("row ")) == int(want["rows"])
    res = subprocess.run([cli, "compare", path("a.lac"), path("d.lac")], capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and res.stdout == "" and res.stderr.startswith("Compare failed: channel counts differ (1, 2)")
    res = subprocess.run([cli, "compare", path("a.lac")], capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and "lacx_cli compare A B" in res.stderr
