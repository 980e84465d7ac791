"""Stream inspection on the MI355X: lacx_decoder_inspect_batch_device, lacx_decoder_item_block_info,
lacx_decoder_item_partitions and `lacx_cli inspect` against tests/lacinspect.py, the walk restated in plain Python -- never
the code under test.  Equality is exact for every field of every row, every partition entry and every report.  Whatever
goes to the device has first passed the sanitized CPU twin of the job (tests/native/sim_inspect.cpp, every buffer at
exactly the plan's capacity) in this run."""
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import inspectcorpus as ic
import inspecttwin as tw
import lacgrammar as g
import lacinspect as li
import lacmutate
import lacstreams
import narrowrecipes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "lossless-audio-codec_amd")
FINALS = (1, 255, 256, 257, 4097, 16384)
FORMATS = ((1, 16, 44100, 0), (1, 24, 96000, 0), (2, 16, 48000, 0), (2, 16, 44100, 1), (2, 24, 48000, 2), (2, 24, 192000, 1), (2, 16, 96000, 2))


@pytest.fixture(scope="module")
def gpu():
    pkg = ge.load_pkg()
    if pkg.lacx.device_count() <= 0:
        pytest.fail("no HIP device: the decoder has no CPU fallback")
    return pkg


def _info(lac):
    return (lac[2], lac[3], lac[4], lac[6] | (lac[5] << 8) | (lac[7] << 16), lac[8], struct.unpack(">I", lac[10:14])[0])


def _check(what, got, lac, partitions=False):
    """One item of an inspection call against the reference: the rows (and partition entries), the identities on every
    block that parses, and the report."""
    report, rows = got
    want = ic.expected(lac)
    have = [li.from_ctypes(r) for r in rows]
    want_rows = want if partitions else li.strip_partitions(want)
    assert have == want_rows, (what, li.diff(have, want_rows))
    for r in have:
        if r["code"] == 0:
            li.check_identities(r, ic.stereo_flag(lac))
    assert li.report_from_ctypes(report) == li.report(want, _info(lac)), what


def _batch(gpu, key, lacs, partitions=False, stream=0, dec=None):
    """lacs through the sanitized twin, then as one device job; BatchDecodeError never: these containers are all accepted."""
    lacs = tw.cleared(key, list(lacs))
    own = dec is None
    dec = dec or gpu.lacx.Decoder(device=0)
    got = dec.inspect_batch(lacs, partitions=partitions, stream=stream)
    assert dec.last_ms > 0
    if own:
        dec.close()
    return got


def test_pinned_streams_shuffled_and_one_at_a_time(gpu):
    """The 26 pinned streams (version 2 and spliced ones among them) as one shuffled batch with duplicates, then singly."""
    lacs = [l for _, l in ic.pinned()]
    assert len(lacs) == 26
    rng = random.Random(11)
    order = lacs + [rng.choice(lacs) for _ in range(14)]
    rng.shuffle(order)
    for k, (lac, got) in enumerate(zip(order, _batch(gpu, "pinned", order, partitions=True))):
        _check("batch %d" % k, got, lac, True)
    dec = gpu.lacx.Decoder(device=0)
    for name, lac in ic.pinned():
        got = dec.inspect_batch([lac])
        _check(name, got[0], lac)
        assert bytes(dec.inspect(lac)) == bytes(got[0][0])
    dec.close()


def test_grammar_failing_cases_included_as_one_batch(gpu):
    """All of lacgrammar (the wave mixes among it) as one job: every block's verdict and tally, the failing cases' codes
    beside their neighbours' rows."""
    cases = ic.grammar()
    got = _batch(gpu, "grammar", [lac for _, lac, _, _ in cases], partitions=True)
    codes = set()
    for (name, lac, status, bad), item in zip(cases, got):
        _check(name, item, lac, True)
        codes |= {r.code for r in item[1]}
        if status not in (0, 5, 7):
            assert item[1][bad].code == status, name
    assert {0, 1, 2, 3, 4, 6, 9} <= codes and not codes & {5, 7}
    assert all(name in dict((c[0], 1) for c in cases) for name in g.WAVE_MIXES)


def test_failure_mix_shares_waves(gpu):
    """96 single-block streams in two waves, every fifth refused: each reports its own code, its neighbours their rows."""
    mix = g.failure_mix()
    got = _batch(gpu, "failure_mix", [s.lac for _, s in mix])
    for i, ((name, s), item) in enumerate(zip(mix, got)):
        _check("mix %d" % i, item, s.lac)
        assert (item[1][0].code != 0) == (name is not None and s.status not in (5, 7)), (i, name)


@pytest.fixture(scope="module")
def encoded(gpu):
    """Streams of the device encoder: every format with every final block size, and per format one of two blocks."""
    out = []
    for k, (ch, depth, rate, sm) in enumerate(FORMATS):
        enc = gpu.lacx.Encoder(12, sm, rate, depth, device=0)
        for frames in FINALS + (16384 + 257,):
            left, right = gpu.synth.synth_pcm(frames, ch, depth, rate, seed=300 + 7 * k + frames % 11, kind=("music", "mixed", "noise", "tone")[(k + frames) % 4])
            out.append(("%dch%d sm%d n%d" % (ch, depth, sm, frames), enc.encode(left, right)))
    return out


def test_encoded_streams_of_every_format(gpu, encoded):
    got = _batch(gpu, "encoded", [lac for _, lac in encoded])
    finals = set()
    for (name, lac), item in zip(encoded, got):
        _check(name, item, lac)
        assert item[0].lost_blocks == 0
        finals.add(item[1][-1].frames)
    assert finals == set(FINALS) | {257}
    assert {(lac[3], lac[4], lac[8]) for _, lac in encoded} == {(c, s, d) for c, d, _, s in FORMATS}


def test_partition_of_exactly_32_and_lpc_order_32(gpu):
    """A block of 8192 samples at partition order 8 (n >> p == 32, the smallest partition the format allows) under an LPC
    predictor of order 32, and the same at a final block of 8192 + 31 (the last partition takes the remainder)."""
    rng = random.Random(32)
    lacs = []
    for n in (8192, 8223):
        samples = g.walk(rng, n, 40, -30000, 30000)
        cb = g.block_of(samples, ptype=2, order=32, coefs=g.rand_coefs(rng, 32, 900), porder=8,
                        modes=(g.MODE_STATIC, g.MODE_RICE, g.MODE_ZERO_RUN, g.MODE_BIN), seed=n)
        lacs.append(g.mono(cb).lac)
    got = _batch(gpu, "p8o32", lacs, partitions=True)
    for lac, item in zip(lacs, got):
        _check("p8 o32", item, lac, True)
        c = item[1][0].ch[0]
        assert item[1][0].code == 0 and (c.order, c.partition_order, c.partitions) == (32, 8, 256) and item[1][0].frames >> 8 == 32
        assert len(item[1][0].partitions[0]) == 256 and any(c.coef[31:32])


def test_partition_detail_on_and_off(gpu, encoded, monkeypatch):
    """The same streams with and without LACX_INSPECT_PARTITIONS on one handle: equal rows and reports; the entries are the
    reference's, and without the flag there are none to ask for.  Nothing past the rows is written: with
    LACX_INSPECT_GUARD=1 the bytes behind the job's tables on the device -- 4096, and without the flag also as many as the
    partition entries of all its blocks would take, which is where they would lie -- hold a pattern before the kernels
    run, and every one of them holds it afterwards.  Failing and version-2 streams are in the batch."""
    lacs = [lac for _, lac in encoded[::3]] + [l for _, l in ic.pinned()[:8]] + [lac for _, lac, st, _ in ic.grammar() if st in (1, 2, 3, 4, 6, 9)][:12]
    blocks = sum(len(ic.expected(x)) for x in lacs)
    dec = gpu.lacx.Decoder(device=0)
    assert dec.inspect_guard() == (0, 0)
    plain = _batch(gpu, "onoff", lacs, partitions=False, dec=dec)
    assert dec.inspect_guard() == (0, 0)  # no guard unless asked for
    monkeypatch.setenv("LACX_INSPECT_GUARD", "1")
    on = _batch(gpu, "onoff", lacs, partitions=True, dec=dec)
    assert dec.inspect_guard() == (4096, 0)
    off = _batch(gpu, "onoff", lacs, partitions=False, dec=dec)
    assert dec.inspect_guard() == (4096 + 2560 * blocks + 16, 0)
    fresh = gpu.lacx.Decoder(device=0)  # a buffer that never held a larger job
    again = _batch(gpu, "onoff-few", lacs[:5], partitions=False, dec=fresh)
    assert fresh.inspect_guard() == (4096 + 2560 * sum(len(ic.expected(x)) for x in lacs[:5]) + 16, 0)
    fresh.close()
    monkeypatch.delenv("LACX_INSPECT_GUARD")
    assert [[bytes(r) for r in a[1]] for a in again] == [[bytes(r) for r in a[1]] for a in off[:5]]
    assert [[bytes(r) for r in a[1]] for a in plain] == [[bytes(r) for r in a[1]] for a in off]
    import ctypes as C
    mk, pb, n = C.POINTER(C.c_uint8)(), C.POINTER(C.c_uint32)(), C.c_uint32()
    assert gpu.lacx.lib().lacx_decoder_item_partitions(dec._h, 0, 0, 0, C.byref(mk), C.byref(pb), C.byref(n)) == gpu.lacx.E_INVALID
    for lac, a, b in zip(lacs, on, off):
        _check("on", a, lac, True)
        assert bytes(a[0]) == bytes(b[0]) and [bytes(r) for r in a[1]] == [bytes(r) for r in b[1]]
        assert all(r.partitions is None for r in b[1])
    dec.close()


def test_mutants_of_every_code_and_family_and_truncated_files(gpu, oracle):
    """A seeded selection of damaged streams -- every mutation family, every parse code the corpus reaches -- and files cut
    at every kind of place, in one batch."""
    corpus = lacmutate.corpus(oracle.channel_block_end)
    rng = random.Random(2024)
    by_family = {}
    for m in corpus:
        by_family.setdefault(m.family, []).append(m)
    assert set(by_family) == set(lacmutate.FAMILIES)
    pick = [m for fam in lacmutate.FAMILIES for m in rng.sample(by_family[fam], 36)]
    codes, _ = tw.codes([m.lac for m in corpus[::7]])
    want_codes = {c for cs in codes for c in cs}
    for code in sorted(want_codes):  # one mutant at least for every code the corpus reaches
        k = next(i for i, cs in enumerate(codes) if code in cs)
        pick.append(corpus[7 * k])
    cut = [c for _, l in ic.pinned()[:6] if l[2] == 3 for c in ic.cuts(l)]
    lacs = [m.lac for m in pick] + cut
    got = _batch(gpu, "mutants", lacs)
    seen = set()
    for k, (lac, item) in enumerate(zip(lacs, got)):
        _check("mutant %d" % k, item, lac)
        seen |= {r.code for r in item[1]}
    assert want_codes | {10} <= seen and {0, 1, 2, 3, 4, 6, 9, 10} <= seen, (sorted(seen), sorted(want_codes))
    print("mutants %d, cut files %d, codes %s" % (len(pick), len(cut), sorted(seen)))


def _repeat_block(lac, copies):
    assert lac[2] == 3 and struct.unpack(">I", lac[10:14])[0] == 1
    return lac[:10] + struct.pack(">I", copies) + lac[14:22] * copies + lac[22:] * copies


def test_more_blocks_than_one_resident_round(gpu):
    """More than 32768 blocks of 256 frames in one job: every row of an item is its single block's row."""
    items, ones = [], []
    for k, (ch, bd, rate, sm, kind) in enumerate([(2, 16, 44100, 2, "music"), (1, 24, 96000, 0, "mixed"), (2, 24, 48000, 1, "noise"), (2, 16, 48000, 0, "tone")]):
        left, right = gpu.synth.synth_pcm(256, ch, bd, rate, seed=900 + k, kind=kind)
        one = gpu.lacx.Encoder(12, sm, rate, bd, device=0).encode(left, right)
        ones.append(one)
        items.append(_repeat_block(one, 10007 + 13 * k))
    tw.cleared("round", ones + [_repeat_block(ones[0], 130)])
    dec = gpu.lacx.Decoder(device=0)
    got = dec.inspect_batch(items)
    assert sum(len(rows) for _, rows in got) > 40000
    for one, lac, (report, rows) in zip(ones, items, got):
        want = li.strip_partitions(ic.expected(one))[0]
        assert li.from_ctypes(rows[0]) == want and len(rows) == 10007 + 13 * items.index(lac)
        first = bytes(rows[0])
        assert all(bytes(r) == first for r in rows)
        assert report.blocks == len(rows) and report.lost_blocks == 0 and report.payload_bytes == want["bytes"] * len(rows)
    dec.close()


def test_one_handle_alternating_job_forms(gpu, encoded):
    """Inspect, stats, a window decode and inspect again on one decoder, the inspections on a stream of the caller's."""
    import torch
    lacs = [lac for _, lac in encoded[5:12]]
    dec = gpu.lacx.Decoder(device=0)
    side = torch.cuda.Stream()
    first = _batch(gpu, "alt", lacs, partitions=True, stream=side.cuda_stream, dec=dec)
    stats = dec.stats_batch(lacs)
    info = gpu.lacx.stream_parse(lacs[-1])
    win = dec.decode_window(lacs[-1], 100, min(1000, info.frames - 100))
    want_l, want_r, _, _ = gpu.lacx.decode(lacs[-1])
    assert np.array_equal(np.asarray(win[0]).reshape(-1), want_l[100:100 + min(1000, info.frames - 100)])
    again = _batch(gpu, "alt", lacs, partitions=False, stream=side.cuda_stream, dec=dec)
    side.synchronize()
    for lac, a, b, s in zip(lacs, first, again, stats):
        _check("alt", a, lac, True)
        assert bytes(a[0]) == bytes(b[0]) and [bytes(r) for r in a[1]] == [bytes(r) for r in b[1]]
        assert s[0].frames == a[0].frames and len(s[1]) == len(a[1])
    dec.close()


def test_the_encoders_plan_records_read_back_out_of_its_bytes(gpu):
    """The loop closed: for the narrowrecipes streams encoded by the device encoder, every field that both
    lacx_channel_plan (Encoder.analyze) and the inspection rows of the encoder's own output define is equal."""
    compared = ("predictor_type", "order", "coef", "partition_order", "part_mode_k", "payload_bytes * 8 == bits")
    streams = narrowrecipes.streams() + narrowrecipes.stereo_streams()
    count = 0
    lacs, plans = [], []
    for k, (name, depth, left, right) in enumerate(streams):
        enc = gpu.lacx.Encoder(12, (2, 1, 0)[k % 3], 48000, depth, device=0)
        plans.append(enc.analyze(left, right))
        lacs.append(enc.encode(left, right))
    got = _batch(gpu, "loop", lacs, partitions=True)
    for (name, *_), lac, (bplans, cplans), (report, rows) in zip(streams, lacs, plans, got):
        assert report.lost_blocks == 0 and len(rows) == len(bplans), name
        for b, row in enumerate(rows):
            for c in range(row.channels):
                plan, info = cplans[16 * b + (2 + c if row.ms else c)], row.ch[c]
                where = (name, b, c)
                assert plan.valid, where
                assert (plan.predictor_type, plan.order, plan.partition_order) == (info.predictor_type, info.order, info.partition_order), where
                assert list(plan.coef) == list(info.coef)[:12] and not any(list(info.coef)[12:]), where
                assert [mk for mk, _ in row.partitions[c]] == list(plan.part_mode_k)[:info.partitions], where
                assert plan.payload_bytes * 8 == info.bits, where
                count += 1
    print("channel blocks compared:", count, "fields:", ", ".join(compared))
    assert count == sum(len(rows) * lac[3] for lac, (_, rows) in zip(lacs, got)) and count > 0


def test_cli_inspect(gpu, tmp_path, encoded):
    """One line of integers per file, block and partition lines with the flags, a damaged stream's line with exit 0, and a
    refused container on stderr with exit 1."""
    cli = os.path.join(PKG_DIR, "lacx_cli")
    good, cut = encoded[6][1], ic.cuts(ic.pinned()[0][1])[-1]
    tw.cleared("cli", [good, cut])
    for name, data in (("good.lac", good), ("cut.lac", cut), ("bad.lac", b"LA\x03\x02")):
        (tmp_path / name).write_bytes(data)
    res = subprocess.run([cli, "inspect", str(tmp_path / "good.lac"), str(tmp_path / "cut.lac"), "--blocks", "--partitions"], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.splitlines()
    heads = [ln for ln in lines if ln.startswith("frames=")]
    assert len(heads) == 2
    for head, lac in zip(heads, (good, cut)):
        t = li.report(ic.expected(lac), _info(lac))
        fields = dict(f.split("=") for f in head.split() if "=" in f)
        assert int(fields["blocks"]) == t["blocks"] and int(fields["lost_blocks"]) == t["lost_blocks"] and int(fields["payload_bytes"]) == t["payload_bytes"]
        assert [int(x) for x in fields["mode_samples"].split(",")] == t["mode_samples"] and int(fields["unary_bits"]) == t["unary_bits"]
        assert int(fields["sum_u"]) == t["sum_u"]
    assert int(dict(f.split("=") for f in heads[1].split() if "=" in f)["lost_blocks"]) >= 1
    nblocks = sum(len(ic.expected(x)) for x in (good, cut))
    assert sum(ln.startswith("  block=") for ln in lines) == nblocks
    assert sum(ln.startswith("    block=") for ln in lines) == sum(sum(c["mode_parts"]) for x in (good, cut) for r in ic.expected(x) for c in r["ch"])
    res = subprocess.run([cli, "inspect", str(tmp_path / "bad.lac"), str(tmp_path / "good.lac")], capture_output=True, text=True)
    assert res.returncode == 1 and "invalid frame header" in res.stderr and len(res.stdout.splitlines()) == 1
