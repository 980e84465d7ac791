"""The rip-checksum entry points without a device: the new structs against the library's own sizeof, the plan's split and
tile counts, the disc ids against plain Python (tests/artwin.py), the two restatements of the sums against each other and
against Python integers, the per-disc refusals -- each made on the host before any device work -- and the refusal of the job
beside the other jobs of the digest form."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
import artwin as aw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ("lacx_decoder_accuraterip_batch_device", "lacx_decoder_accuraterip_pcm_batch_device", "lacx_decoder_item_ar_tracks", "lacx_decoder_item_ar_sums",
       "lacx_ar_ids")
FAKE = 1 << 40  # a "device address" that is never dereferenced: every call here stops before the device


@pytest.fixture(scope="module")
def pkg():
    mod = ge.load_pkg()
    if not os.path.exists(mod.lacx.LIB_PATH):
        mod.lacx.build()
    return mod


def _fixture(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def test_symbols_and_structs(pkg):
    L, lx = pkg.lacx.lib(), pkg.lacx
    header = open(os.path.join(ROOT, "include", "lacx.h")).read()
    for name in NEW:
        assert hasattr(L, name) and name in lx.EXPORTS
        assert re.search(rf"\b{name}\s*\(", header), name
        assert header.index(name) < header.index("#ifndef LACX_H"), name  # listed in the comment block at the top
    structs = lx.abi_structs()
    for name, cls, size in (("ar_disc", lx.ArDisc, 28), ("ar_id", lx.ArId, 12), ("ar_result", lx.ArResult, 32), ("ar_track", lx.ArTrack, 32)):
        assert structs[name] is cls and L.lacx_sizeof(name.encode()) == C.sizeof(cls) == size, name
    assert C.sizeof(lx.ArTrack) == aw.TRACK_T.itemsize and C.sizeof(lx.ArResult) == aw.RESULT_T.itemsize
    assert (lx.AR_FIRST, lx.AR_LAST, lx.AR_NO_IDS, lx.AR_TRACK_SHORT, lx.AR_TRACK_NO_S450) == (aw.FIRST, aw.LAST, aw.NO_IDS, aw.TRACK_SHORT, aw.TRACK_NO_S450)
    assert lx.AR_MAX_RADIUS == aw.MAX_RADIUS == 5 * aw.SECTOR - 1


def test_the_plans_split_and_tiles():
    """Offsets per tile: the smallest power of two that holds 2 radius + 1, at most 256 -- the radii of the corpus fall on
    both sides of every border; a disc's tiles are, per span, multiplier tiles of 4096 times offset tiles."""
    assert [aw.lib().sim_ar_lanes(r) for r in aw.RADII] == [1, 4, 64, 128, 256, 256, 256, 256]
    assert [aw.lib().sim_ar_lanes(r) for r in (2, 3, 4, 15, 16, 63, 64)] == [8, 8, 16, 32, 64, 128, 256]
    M = aw.lib().sim_ar_tile_mults()
    assert M == 4096 and set(aw.TILE_LENGTHS) >= {M - 1, M, M + 1, 2 * M, 2 * M + 1}

    def tiles(tracks, first, last, radius):
        d = aw.Disc("x", [], tracks, radius, first, last)
        lanes = aw.lib().sim_ar_lanes(radius)
        ot = (2 * radius + lanes) // lanes
        total = 0
        for start, n, lo, hi, flags in aw.ranges(d):
            total += ((hi - lo) // M + 1) * ot if hi >= lo else 0
            total += ot if not flags & aw.TRACK_NO_S450 else 0
        return total

    for tracks, first, last, radius in ((aw.THREE, True, True, 0), (aw.THREE, True, True, 128), (aw.THREE, False, False, 2939), ((4096,), False, False, 0),
                                        ((4097,), False, False, 0), ((2939,), True, True, 5), ((aw.BIG,), True, True, 2939), ((aw.BIG, 5), True, True, 127)):
        assert aw.twin_tiles(tracks, first, last, radius) == tiles(tracks, first, last, radius), (tracks, radius)
    assert aw.twin_tiles((4096,), False, False, 0) == 1 and aw.twin_tiles((4097,), False, False, 0) == 2
    assert aw.twin_tiles((aw.BIG,), True, True, 2939) == (((aw.BIG - 2 * aw.EDGE) // M + 1) + 1) * 23
    assert aw.twin_tiles((0, 5), True, True, 0) == aw.twin_tiles((5,), True, True, 2940) == aw.twin_tiles((1,) * 100, True, True, 0) == -1


def test_ids_against_plain_python(pkg):
    """lacx_ar_ids, the plan's ar_ids (through the twin) and the Python restatement agree; a worked example by hand."""
    lx = pkg.lacx
    # three tracks of 12, 10 and 15 sectors from lba 32: lba = 32, 44, 54, leadout 69
    hand = aw.expected_ids((588 * 12, 588 * 10, 588 * 15), True, True, 32)
    assert hand.id1 == 32 + 44 + 54 + 69 and hand.id2 == 32 * 1 + 44 * 2 + 54 * 3 + 69 * 4
    assert hand.cddb == (((2 + 2 + 2) % 255) << 24) | (((69 + 150) // 75 - (32 + 150) // 75) << 8) | 3  # 182 // 75 = 2, 194 // 75 = 2, 204 // 75 = 2
    g = np.random.default_rng(77)
    cases = [((588 * 12, 588 * 10, 588 * 15), True, True, 32), ((588,), True, True, 0), ((588 * 20000, 588 * 15000), True, True, 150)]
    cases += [(tuple(int(v) * 588 for v in g.integers(1, 30000, int(g.integers(1, 100)))), True, True, int(g.integers(0, 400))) for _ in range(20)]
    cases += [((588, 589), True, True, 0), ((588, 588), False, True, 0), ((588, 588), True, False, 0), (aw.THREE, True, True, 0)]
    for tracks, first, last, lba0 in cases:
        want = aw.expected_ids(tracks, first, last, lba0)
        got = lx.ar_ids(tracks, first, last, lba0)
        has, twin = aw.twin_ids(tracks, first, last, lba0)
        assert (got.id1, got.id2, got.cddb) == tuple(want) == tuple(twin), (tracks, lba0)
        assert has == (first and last and all(n % 588 == 0 for n in tracks))
    for tracks, text in (((), "disc has no tracks"), ((1,) * 100, "more than 99 tracks"), ((5, 0), "track 1 is empty")):
        with pytest.raises(ValueError, match=re.escape(text)):
            lx.ar_ids(tracks)
    out = lx.ArId()
    assert lx.lib().lacx_ar_ids((C.c_uint64 * 1)(588), 1, 8, 0, C.byref(out)) == lx.E_INVALID and lx.lib().lacx_decode_last_error() == b"unknown flags"


def test_the_two_restatements_agree():
    """The definition in uint64 products and the prefix sums give the same v1 and s450 on every small disc of the corpus; v2 is
    Python integers' at a handful of (track, offset) pairs; with both flags no sum reads outside the disc."""
    for d in aw.small_corpus():
        e = aw.expected(d)
        v1, s450 = aw.expected_prefix(d)
        assert (e.v1 == v1).all() and (e.s450 == s450).all(), d.name
    by = {d.name: d for d in aw.corpus()}
    for name, picks in (("three|r300", ((0, -300), (1, 0), (2, 300), (1, 7))), ("flags|00", ((0, -300), (2, 300))), ("ones", ((0, 0), (2, -128))),
                        ("lowest", ((1, 128),)), ("seams", ((0, -299), (1, 300)))):
        d = by[name]
        for t, o in picks:
            assert int(aw.expected(d).v2[t][o + d.radius]) == aw.v2_bigint(d, t, o), (name, t, o)
    three = by["three|r2939"]
    D = sum(aw.THREE)
    reads = [(s + o + lo - 1, s + o + hi - 1) for s, n, lo, hi, _ in aw.ranges(three) for o in (-2939, 2939)]
    assert min(a for a, _ in reads) == 0 and max(b for _, b in reads) == D - 2


def test_refusals_before_any_device_work(pkg):
    """Every host refusal of a disc, with its text (no disc here is in order: nothing reaches a device), the
    call's own arguments checked too.  The stream form parses its streams; the source form never
    touches its addresses."""
    lx = pkg.lacx
    dec = lx.Decoder()
    good = (FAKE, FAKE + (1 << 20), aw.P32, 2, 1000)
    src = lambda pcm=good, rate=44100, depth=16: (pcm, rate, depth)  # noqa: E731
    discs = [([], None, 0),
             ([src()], (1,) * 100, 0),
             ([src()], (1000, 0), 0),
             ([src(), src()], (1000, 999), 0),
             ([src()], None, 2940),
             ([src(rate=48000)], None, 0),
             ([src(), src(depth=24)], None, 0),
             ([src(), src((FAKE, None, aw.P32, 1, 1000))], None, 0),
             ([src((FAKE, FAKE, 7, 2, 1000))], None, 0)]
    with pytest.raises((lx.BatchDecodeError, RuntimeError)):  # (every disc is refused: nothing reaches a device, with or without one)
        dec.accuraterip_pcm_batch(discs)
    want = {0: "disc has no sources", 1: "more than 99 tracks", 2: "track 1 is empty", 3: "track lengths do not sum to the disc's frames (1999, 2000)",
            4: "radius above 2939", 5: "source 0: not CD audio (2 channels, 16 bit, 48000 Hz)", 6: "source 1: not CD audio (2 channels, 24 bit, 44100 Hz)",
            7: "source 1: not CD audio (1 channels, 16 bit, 44100 Hz)", 8: "source 0: unknown source layout"}
    L = lx.lib()
    for k, text in want.items():
        assert L.lacx_decoder_item_error(dec._h, k).decode() == text, k
    # unknown flags and arrays outside the call's, through the C interface
    one = (lx.DigestSource * 1)()
    one[0].pcm, one[0].frames, one[0].sample_rate, one[0].bit_depth = lx.Pcm(FAKE, FAKE, aw.P32, 2), 1000, 44100, 16
    recs = (lx.ArDisc * 4)(lx.ArDisc(0, 1, 0, 0, 8, 0, 0), lx.ArDisc(1, 1, 0, 0, 3, 0, 0), lx.ArDisc(0, 1, 1, 1, 3, 0, 0), lx.ArDisc(0, 2, 0, 0, 3, 0, 0))
    rcs, out, tf = (C.c_int * 4)(), (lx.ArResult * 4)(), (C.c_uint64 * 1)(1000)
    rc = L.lacx_decoder_accuraterip_pcm_batch_device(dec._h, one, 1, tf, 1, recs, 4, None, rcs, out, None)
    assert rc != lx.OK and list(rcs) == [lx.E_INVALID] * 4 and bytes(out) == bytes(C.sizeof(out))
    assert [L.lacx_decoder_item_error(dec._h, k).decode() for k in range(4)] == ["unknown flags", "sources outside the call's array",
                                                                                 "tracks outside the call's array", "sources outside the call's array"]
    assert L.lacx_decoder_accuraterip_pcm_batch_device(dec._h, one, 1, tf, 1, recs, 0, None, rcs, out, None) == lx.E_INVALID
    assert L.lacx_decoder_accuraterip_pcm_batch_device(None, one, 1, tf, 1, recs, 1, None, rcs, out, None) == lx.E_INVALID
    ptr, count = C.POINTER(lx.ArTrack)(), C.c_uint32(9)
    assert L.lacx_decoder_item_ar_tracks(dec._h, 0, C.byref(ptr), C.byref(count)) == lx.E_INVALID and count.value == 0
    # the stream form: a stream that does not parse, one that is no CD audio (24 bit, 48 kHz mono fixtures)
    st16 = _fixture("decode_wav/st16_lr_3blk.lac")
    info = lx.stream_parse(st16)
    spans_of = lambda xs: (lx.Span * len(xs))(*[lx.Span(C.cast(C.c_char_p(x), C.POINTER(C.c_uint8)), len(x)) for x in xs])  # noqa: E731
    keep = [st16, b"XX" + st16[2:], st16[:12]]
    recs = (lx.ArDisc * 3)(lx.ArDisc(1, 1, 0, 0, 3, 0, 0), lx.ArDisc(0, 2, 0, 0, 3, 0, 0), lx.ArDisc(2, 1, 0, 0, 3, 0, 0))
    rcs3, out3 = (C.c_int * 3)(), (lx.ArResult * 3)()
    rc = L.lacx_decoder_accuraterip_batch_device(dec._h, spans_of(keep), 3, None, 0, recs, 3, None, rcs3, out3, None)
    assert rc != lx.OK and all(v != lx.OK for v in rcs3) and bytes(out3) == bytes(C.sizeof(out3))
    texts = [L.lacx_decoder_item_error(dec._h, k).decode() for k in range(3)]
    assert (info.channels, info.bit_depth, info.sample_rate) == (2, 16, 48000)  # the fixture is no CD audio: its disc is refused for that
    assert texts[0] == "source 0: [decode-error] invalid frame header" and texts[1] == "source 0: not CD audio (2 channels, 16 bit, 48000 Hz)"
    assert texts[2].startswith("source 0: [decode-error] ") and rcs3[1] == lx.E_INVALID
    dec.close()


def test_the_job_is_refused_beside_the_other_digest_form_jobs():
    """decode_plan.h: a rip-checksum job is a strict job in the digest form and shares it with no other job; every existing
    caller's plan_decode compiles unchanged (the new parameter is defaulted: the twins of the other jobs build from the same
    header)."""
    plan = open(os.path.join(ROOT, "lossless-audio-codec_amd", "csrc", "decode_plan.h")).read()
    assert 'if (ar && (!digest || salvage || loudness || truepeak || spectrum)) return "rip checksums are a strict job in the digest form";' in plan
    assert "uint32_t spectrum = 0, const ArJobIn* ar = nullptr)" in plan
    host = open(os.path.join(ROOT, "lossless-audio-codec_amd", "csrc", "accuraterip_plan.h")).read()
    assert "hip" not in host.replace("no HIP", "").replace(".hip", "").lower().replace("ship", "")
