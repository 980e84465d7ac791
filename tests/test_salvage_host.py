"""The salvage decode (decode through errors) without a device: the lenient parse (lacx_stream_scan), the salvage plan
(csrc/decode_plan.h) and the CPU twin of the whole job (tests/native/sim_salvage.cpp: the lane code, ms_inverse_tile and
csrc/salvage_core.h over buffers of exactly the plan's capacities, plain and under AddressSanitizer + UBSan as a program of
its own) against salvagetwin.expected(), which asks the oracle block by block and never the code under test.

The corpus: every lacmutate mutant whose base has at least two blocks, every version-2 mutant, a truncation family (each
such base cut inside every block and exactly at every border) and a stream stitched from 257-frame blocks, damaged and cut,
so that lost and decoded blocks meet at frame indices that are no multiple of four."""
import collections
import ctypes as C
import glob
import os
import struct

import numpy as np
import pytest

import dectwin
import lacmutate
import lacstreams
import mutantjudge
import salvagetwin as st

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LENGTH_MESSAGES = ("[decode-error] block payloads do not fill the file", "[decode-error] compressed block sizes exceed frame payload")


def _read(path):
    with open(path, "rb") as f:
        return f.read()


FIXTURES = {os.path.basename(p)[:-4]: _read(p) for d in ("small", "decode_wav") for p in sorted(glob.glob(os.path.join(GOLDEN, d, "*.lac")))}


def _scan(lacx, buf, size):
    """lacx_stream_scan of the first `size` bytes of a uint8 array, without copying it -> (rc, info, present, flags, message)."""
    info, present, flags = lacx.StreamInfo(), C.c_uint32(), C.c_uint32()
    rc = lacx.lib().lacx_stream_scan(buf.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_uint64(size), C.byref(info), C.byref(present), C.byref(flags))
    return rc, info, present.value, flags.value, "" if rc == 0 else lacx.lib().lacx_decode_last_error().decode()


def _info(i):
    return (i.sample_rate, i.blocks, i.frames, i.channels, i.bit_depth, i.stereo_mode, i.version)


def _parse_message(lacx, lac):
    info = lacx.StreamInfo()
    buf = (C.c_uint8 * max(1, len(lac))).from_buffer_copy(lac if lac else b"\0")
    rc = lacx.lib().lacx_stream_parse(buf, C.c_uint64(len(lac)), C.byref(info))
    return "" if rc == 0 else lacx.lib().lacx_decode_last_error().decode()


# ---- the lenient parse ------------------------------------------------------------------------------------------------
def test_scan_accepts_what_parse_accepts(pkg, oracle):
    """Every stream stream_parse accepts: the same info, every block present, no flag."""
    lacx = pkg.lacx
    streams = dict(lacmutate.bases(oracle.channel_block_end))
    streams.update(FIXTURES)
    for name, lac in streams.items():
        want = lacx.stream_parse(lac)
        assert want is not None, name
        info, present, flags = lacx.stream_scan(lac)
        assert _info(info) == _info(want) and present == want.blocks and flags == 0, name


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_scan_of_every_truncation_and_of_appended_bytes(pkg, name):
    """A fixture cut at every byte from the end of its table to its end: the info of the whole stream, the present
    blocks the table implies, TRUNCATED; below the table's end the strict parser's refusal; bytes appended: TRAILING."""
    lacx = pkg.lacx
    lac = FIXTURES[name]
    whole = lacx.stream_parse(lac)
    _, ent, head = lacmutate.table(lac)
    ends = np.cumsum([s for _, s in ent]) + head
    buf = np.frombuffer(lac + b"\xa5" * 40, dtype=np.uint8)
    for size in range(head, len(lac)):
        rc, info, present, flags, _ = _scan(lacx, buf, size)
        assert rc == 0 and _info(info) == _info(whole), (name, size)
        assert present == int(np.searchsorted(ends, size, side="right")) and flags == st.TRUNCATED, (name, size, present)
    for size in range(0, head):
        rc, _, present, flags, msg = _scan(lacx, buf, size)
        assert rc != 0 and (present, flags) == (0, 0) and msg == _parse_message(lacx, lac[:size]), (name, size, msg)
        assert msg not in LENGTH_MESSAGES
    for extra in (1, 2, 17, 40):
        rc, info, present, flags, _ = _scan(lacx, buf, len(lac) + extra)
        assert rc == 0 and _info(info) == _info(whole) and present == whole.blocks and flags == st.TRAILING, (name, extra)


def test_scan_refuses_damaged_heads_with_the_strict_message(pkg):
    """Every single-bit flip and every byte value 0x00 / 0xFF in header and block table of the fixtures: what stream_parse
    refuses for a reason other than the payload's length, stream_scan refuses with the same text; the rest it accepts."""
    lacx = pkg.lacx
    refused = collections.Counter()
    accepted = 0
    for name, lac in FIXTURES.items():
        _, _, head = lacmutate.table(lac)
        for pos in range(head):
            for value in [lac[pos] ^ (1 << bit) for bit in range(8)] + [0x00, 0xFF]:
                if value == lac[pos]:
                    continue
                m = lac[:pos] + bytes([value]) + lac[pos + 1:]
                strict = _parse_message(lacx, m)
                got = lacx.stream_scan(m)
                if strict and strict not in LENGTH_MESSAGES:
                    assert got is None and lacx.lib().lacx_decode_last_error().decode() == strict, (name, pos, value, strict)
                    refused[strict] += 1
                elif got is not None:
                    accepted += 1
    print("refused heads by message:", dict(refused), "accepted:", accepted)
    assert len(refused) >= 4 and accepted > 100
    for msg in LENGTH_MESSAGES:
        assert msg not in refused
    assert lacx.stream_scan(b"") is None and lacx.lib().lacx_decode_last_error().decode() == "[decode-error] empty input"


# ---- the plan ---------------------------------------------------------------------------------------------------------
def _up(v, a):
    return (v + a - 1) // a * a


@pytest.mark.parametrize("device", [False, True])
def test_salvage_plan_layout(device):
    """A mixed job -- whole, cut at a border, cut inside a block, cut inside the first block, trailing bytes, version 2, one
    refused table -- planned as the product plans it: lanes for present blocks only, payload = the present blocks'
    bytes, the capacities, the present table, the byte offsets of missing blocks."""
    three, two, mono = FIXTURES["st16_lr_3blk"], FIXTURES["st24_ms_20481"], FIXTURES["mono16_16639"]
    cuts = dict(st.truncations(three))
    v2 = lacstreams.to_v2(three)
    lacs = [three, cuts["border2"], b"LA\x03" + bytes(29), cuts["in1.mid"], cuts["in0.first"], two + b"xyz", v2, mono[:-1]]
    p = st.plan_dump(lacs, device=device)
    assert p["rc"] == [0, 0, 1, 0, 0, 0, 0, 0] and p["msg"][2] == "[decode-error] invalid frame header"
    assert p["m"] == 7 and [it["src"] for it in p["items"]] == [0, 1, 3, 4, 5, 6, 7]
    want_present = [3, 2, 1, 0, 2, 3, 1]
    want_flags = [0, 1, 1, 1, 2, 0, 1]
    lanes, pay, blocks, frames, pcm, image, units = [], 0, 0, 0, 0, 0, 0
    for j, it in enumerate(p["items"]):
        lac = lacs[it["src"]]
        version, ent, head = lacmutate.table(lac)
        assert (it["present"], it["flags"]) == (want_present[j], want_flags[j]), j
        assert int(p["present"][j]) == want_present[j]
        assert it["blocks"] == len(ent) and it["frames"] == sum(n for n, _ in ent) and it["block0"] == blocks and it["head"] == head
        bytes_present = len(lac) - head if version == 2 else sum(s for _, s in ent[:it["present"]])
        assert it["pay_bytes"] == bytes_present and it["pay_off"] == pay
        assert head + bytes_present <= len(lac)  # the device never gets a byte the file does not have
        if version == 3:
            lanes += list(range(blocks, blocks + it["present"]))
            for b in range(len(ent)):
                step = ent[b][1] if b < it["present"] else 0
                assert int(p["byte_off"][blocks + b + 1]) - int(p["byte_off"][blocks + b]) == step
            assert int(p["byte_off"][blocks]) == pay
        rec = p["item"][j]
        if device:
            assert int(rec["left"]) == dectwin.base(4, it["src"]) and int(rec["right"]) == (dectwin.base(5, it["src"]) if lac[3] == 2 else 0)
            assert int(rec["wav"]) == 0
        else:
            assert it["pcm_at"] == pcm and it["image_at"] == image
            assert it["image_size"] == 44 + _up(it["frames"] * lac[3] * (lac[8] // 8), 2)
            assert int(rec["left"]) == dectwin.base(1) + 4 * pcm and int(rec["wav"]) == dectwin.base(3) + image and image % 16 == 0
            pcm += _up(it["frames"], 4)
            image += _up(it["image_size"], 16)
            units += (it["frames"] + 3) // 4
            assert int(p["unit_off"][j + 1]) == units
        assert int(rec["blocks"]) == it["blocks"] and int(rec["frames"]) == it["frames"]
        pay += bytes_present
        blocks += it["blocks"]
        frames += it["frames"]
    assert p["lane_blk"].tolist() == lanes and p["v2_items"].tolist() == [5]
    assert (p["total_blocks"], p["total_frames"], p["total_pay"]) == (blocks, frames, pay)
    assert p["need_payload"] == pay + p["tail_pad"] and p["need_blocks"] == blocks and p["need_stage"] == 0
    assert p["need_pcm"] == (0 if device else pcm) and p["need_image"] == (0 if device else image)
    assert p["o_present"] % 16 == 0 and p["o_present"] >= p["o_v2"] + 4 and p["need_tables"] == p["o_size"] == p["o_present"] + 4 * p["m"]
    assert int(p["frame_off"][blocks]) == frames


# ---- the twin against expected() --------------------------------------------------------------------------------------
def _nblocks(lac):
    return struct.unpack(">I", lac[10:14])[0]


@pytest.fixture(scope="module")
def corpus(oracle, pkg):
    """[(name, stream, the decode twin's per-block statuses of the stream -- of its uncut parent for a cut one)]."""
    records, failures, _ = mutantjudge.judge(oracle, pkg.lacx.stream_parse)
    assert not failures, failures[:5]
    bases = lacmutate.bases(oracle.channel_block_end)
    multi = {name for name, lac in bases.items() if _nblocks(lac) >= 2}
    out = [(r.mutant.name, r.mutant.lac, r.status) for r in records if r.mutant.base in multi or r.mutant.lac[2] == 2]
    for name in sorted(multi):
        if bases[name][2] == 3:
            status = dectwin.decode(bases[name]).status
            out += [("%s|cut|%s" % (name, par), t, status) for par, t in st.truncations(bases[name])]
    return out + st.constructed()


@pytest.fixture(scope="module")
def judged(oracle, corpus):
    """Every corpus entry through the plain twin, both forms, in batches, checked against expected(): per entry
    (name, stream, codes, block frames)."""
    out = []
    for at in range(0, len(corpus), st.BATCH):
        part = corpus[at:at + st.BATCH]
        k = at // st.BATCH
        lacs = [lac for _, lac, _ in part]
        exps = [st.expected(oracle, lac) for lac in lacs]
        wav, over_w = st.run(lacs, device=False, cols=64 if k & 1 else 1, never_lean=bool(k & 2), zero_status=bool(k & 1))
        dev, over_d = st.run(lacs, device=True, cols=1 if k & 1 else 64, never_lean=not (k & 2), zero_status=not (k & 1))
        assert max(over_w, over_d) <= st.DERIVED_OVERSHOOT
        for (name, lac, status), exp, w, d in zip(part, exps, wav, dev):
            assert not w.refused and not d.refused, (name, w.message, d.message)
            st.check(name + " (wav)", lac, exp, status, w.codes, st.result_of(w), image=w.image)
            assert w.image[:44] == b"\xcd" * 44, name  # the header is the host's: the kernel's bytes start behind it
            st.check(name + " (device)", lac, exp, status, d.codes, st.result_of(d), left=d.left, right=d.right)
            out.append((name, lac, w.codes, [n for n, _ in lacmutate.table(lac)[1]]))
    return out


def test_twin_gives_what_the_oracle_expects(judged, corpus):
    """The WAV image byte for byte, the planar arrays, results and fault codes of every corpus entry (the fixture asserts)."""
    print("salvage corpus: %d streams" % len(judged))
    assert len(judged) == len(corpus) and len(judged) > 10000


def test_corpus_is_not_hollow(judged):
    """Every code 1..7 and 9 as a lost block between two decoded ones; 8 and 10; streams that lose their first block, their
    last, two adjacent ones, all of them; a lost block next to a decoded one at a frame index that is no multiple of four."""
    between, codes = collections.Counter(), collections.Counter()
    first = last = adjacent = everything = odd_seam = damaged = clean = 0
    for name, lac, c, frames in judged:
        nb = len(c)
        codes.update(x for x in c if x)
        clean += not any(c)
        damaged += any(c)
        edges = np.concatenate([[0], np.cumsum(frames)])
        for b in range(1, nb - 1):
            if c[b] and not c[b - 1] and not c[b + 1]:
                between[c[b]] += 1
        for b in range(nb - 1):
            if bool(c[b]) != bool(c[b + 1]) and edges[b + 1] % 4:
                odd_seam += 1
        if nb >= 2:
            first += bool(c[0]) and not all(c)
            last += bool(c[-1]) and not all(c)
            adjacent += any(c[b] and c[b + 1] for b in range(nb - 1)) and not all(c)
            everything += all(c)
    print("lost blocks by code:", sorted(codes.items()))
    print("lost between two decoded blocks, by code:", sorted(between.items()))
    print("streams: %d damaged, %d clean; first block lost %d, last %d, two adjacent %d, all %d; seams off a multiple of four %d"
          % (damaged, clean, first, last, adjacent, everything, odd_seam))
    for code in (1, 2, 3, 4, 5, 6, 7, 9):
        assert between[code] >= 1, "no block lost with code %d between two decoded ones" % code
    assert codes[8] >= 1 and codes[10] >= 1
    assert min(first, last, adjacent, everything, odd_seam) >= 1 and clean >= 100 and damaged >= 5000


def test_sanitized_twin_agrees_and_stays_inside_its_buffers(corpus):
    """The same jobs as a program of their own under AddressSanitizer + UBSan: no report with every buffer at exactly the
    plan's capacity, and the plain build's answers."""
    exe, why = st.sanitized_exe()
    if exe is None:
        pytest.skip(why)
    st.cleared("corpus", [lac for _, lac, _ in corpus])


def test_sanitized_program_runs_both_forms():
    """The sanitized program on a clean and a cut stream as one job, WAV form and device form: it ends clean and reports
    the cut stream's last block as missing."""
    exe, why = st.sanitized_exe()
    if exe is None:
        pytest.skip(why)
    lac = FIXTURES["st16_lr_3blk"]
    lines, rc, err = st.run_sanitized([st.case([lac, lac[:-3]]), st.case([lac, lac[:-3]], device=True)], exe)
    assert rc == 0 and len(lines) == 2, err
    for line in lines:
        clean, cut = line.split(" ", 2)[2].split(";")
        assert clean.endswith(" 0 0,0,0") and cut.endswith(" 1 0,0,10"), line
