"""The salvage decode (decode through errors) on the MI355X: lacx_decoder_salvage_wav_batch_view / _salvage_wav /
_salvage_batch_device, the Python binding and `lacx_cli decode --salvage` against salvagetwin.expected(), which asks the
oracle block by block and never the code under test.

The purpose of this module is to CONFIRM WHAT SURVIVES, not to provoke anything: every damaged or cut stream below goes
to the device only after the sanitized CPU twin of the whole salvage job (tests/native/sim_salvage.cpp under
AddressSanitizer + UBSan, every buffer at exactly the plan's capacity, both forms) has passed it in this same run
(salvagetwin.cleared).  Where that build is unavailable the module fails; nothing goes to the device unchecked.

The streams are small: the fixtures, lacmutate's bases of at least three blocks and at most 40 000 frames with a seeded
selection of their mutants, version-2 mutants, cuts at and between block borders, and salvagetwin's constructed streams."""
import collections
import glob
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import dectwin
import lacgrammar as g
import lacmutate
import lacstreams
import salvagetwin as st

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PKG_DIR = os.path.join(ROOT, "lossless-audio-codec_amd")
SENTINEL = 0x5A5A5A5A
EXIT_LOSS = 3  # `decode --salvage`: the file was written, with blocks lost


@pytest.fixture(scope="module")
def gpu():
    pkg = ge.load_pkg()
    if pkg.lacx.device_count() <= 0:
        pytest.fail("no HIP device: the decoder has no CPU fallback")
    return pkg


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _clean_streams():
    out = [(os.path.basename(p)[:-4], _read(p)) for d in ("small", "decode_wav") for p in sorted(glob.glob(os.path.join(GOLDEN, d, "*.lac")))]
    return out + [("v2:" + n, lacstreams.to_v2(lac)) for n, lac in out if n in ("n257_st16_ms", "st16_lr_3blk", "mono24_16641_pad", "n33_mono16")]


CONDITIONS = (["code %d between two decoded blocks" % k for k in (1, 2, 3, 4, 5, 6, 7, 9)] + ["code 8", "code 10"] +
              ["first block lost", "last block lost", "two adjacent blocks lost", "all blocks lost", "a seam off a multiple of four"])
TEXT = {**g.STATUS_TEXT, 8: "not reached", 10: "payload missing"}


def _features(c, frames):
    """The conditions of the host test's corpus that one stream's codes meet."""
    nb = len(c)
    edges = np.concatenate([[0], np.cumsum(frames)])
    out = {"code %d between two decoded blocks" % c[b] for b in range(1, nb - 1) if c[b] and not c[b - 1] and not c[b + 1]}
    out |= {"code %d" % k for k in (8, 10) if k in c}
    if any(bool(c[b]) != bool(c[b + 1]) and edges[b + 1] % 4 for b in range(nb - 1)):
        out.add("a seam off a multiple of four")
    if nb >= 2 and all(c):
        out.add("all blocks lost")
    elif nb >= 2:
        out |= {name for name, ok in (("first block lost", c[0]), ("last block lost", c[-1]),
                                      ("two adjacent blocks lost", any(c[b] and c[b + 1] for b in range(nb - 1)))) if ok}
    return out & set(CONDITIONS)


def _conditions(entries):
    """What keeps the comparison from being hollow, over (codes, block frames) per stream: the conditions not met."""
    have = set()
    for c, frames in entries:
        have |= _features(c, frames)
    return [k for k in CONDITIONS if k not in have]


def _frames(lac):
    return [n for n, _ in lacmutate.table(lac)[1]]


def build_selection(oracle):
    """[(name, stream, the decode twin's statuses or None for a clean fixture)], seeded: mutants of the small bases picked
    for the conditions they add (by the decode twin's statuses) and a few at random, cuts, the constructed streams, clean
    fixtures."""
    rng = random.Random("test_gpu_salvage")
    bases = lacmutate.bases(oracle.channel_block_end)
    small = {n for n, lac in bases.items() if len(_frames(lac)) >= 3 and sum(_frames(lac)) <= 40000}
    assert any(n.startswith("v2:") for n in small) and any(not n.startswith("v2:") for n in small)
    pool = [m for m in lacmutate.corpus(oracle.channel_block_end) if m.base in small]
    rng.shuffle(pool)
    picked, have = [], set()
    for m in pool[:1500]:
        status = dectwin.decode(m.lac).status
        new = _features(status.tolist(), _frames(m.lac)) - have
        if new or (len(picked) < 260 and rng.random() < 0.1):
            have |= new
            picked.append((m.name, m.lac, status))
    for name in sorted(small):
        if bases[name][2] == 3:
            status = dectwin.decode(bases[name]).status
            cuts = list(st.truncations(bases[name]))
            picked += [("%s|cut|%s" % (name, par), t, status) for par, t in rng.sample(cuts, min(6, len(cuts)))]
    picked += st.constructed()
    picked += [(name, lac, None) for name, lac in _clean_streams()]
    rng.shuffle(picked)
    return picked


@pytest.fixture(scope="module")
def selection(gpu, oracle):
    """[(name, stream, expected, the decode twin's statuses)]: a seeded selection that still meets every condition of the
    host test's corpus, with clean streams among the damaged ones -- cleared on the CPU before any of it is used."""
    picked = build_selection(oracle)
    st.cleared("gpu", [lac for _, lac, _ in picked])  # CPU first: nothing below runs if this fails
    return [(name, lac, st.expected(oracle, lac), status) for name, lac, status in picked]


def _codes(nb, faults):
    c = [0] * nb
    for f in faults:
        c[f.block] = f.code
    return c


def _check_faults(name, lac, faults):
    frames = _frames(lac)
    edges = np.concatenate([[0], np.cumsum(frames)])
    assert [f.block for f in faults] == sorted({f.block for f in faults}), name  # ascending, each once
    for f in faults:
        assert (f.frame, f.frames, f.reserved) == (int(edges[f.block]), frames[f.block], 0), (name, f.block)
        assert f.text == TEXT[f.code], (name, f.code)


def _result(r):
    return (r.blocks, r.bad_blocks, r.frames, r.lost_frames, r.first_bad, r.flags)


def test_clean_streams(gpu):
    """Every fixture, versions 3 and 2, as one batch: decode_wav_batch_view's images, no faults, nothing lost."""
    lacs = [lac for _, lac in _clean_streams()]
    dec = gpu.lacx.Decoder(device=0)
    want = [bytes(v) for v in dec.decode_wav_batch_view(lacs)]
    got = dec.salvage_wav_batch(lacs)
    for (name, lac), w, (image, res, faults) in zip(_clean_streams(), want, got):
        assert image == w, name
        nb = len(_frames(lac))
        assert faults == [] and _result(res) == (nb, 0, sum(_frames(lac)), 0, nb, 0), name
    image, res, faults = dec.salvage_wav(lacs[0])
    assert image == want[0] and faults == [] and res.lost_frames == 0
    dec.close()


def test_wav_form(gpu, selection):
    """The selection as batches, clean and damaged items mixed in every job: image, result and fault list of every item."""
    dec = gpu.lacx.Decoder(device=0)
    seen = []
    for at in range(0, len(selection), 128):
        part = selection[at:at + 128]
        got = dec.salvage_wav_batch([lac for _, lac, _, _ in part])
        for (name, lac, exp, status), (image, res, faults) in zip(part, got):
            _check_faults(name, lac, faults)
            codes = _codes(res.blocks, faults)
            st.check(name, lac, exp, status, codes, _result(res))
            assert image == st.wav_image(exp, lac), name  # header, data and pad byte
            seen.append((codes, _frames(lac)))
    dec.close()
    assert not _conditions(seen), _conditions(seen)
    damaged = sum(any(c) for c, _ in seen)
    print("wav form: %d streams, %d damaged" % (len(seen), damaged))
    assert damaged >= 100 and len(seen) - damaged >= 20


def test_device_form(gpu, selection):
    """The same selection into torch int32 tensors pre-filled with a sentinel: a guard element on either side of every array
    is still the sentinel, a mono item's right array is untouched, lost blocks are zero and not sentinel."""
    import torch

    dec = gpu.lacx.Decoder(device=0)
    for at in range(0, len(selection), 128):
        part = selection[at:at + 128]
        tensors = [torch.full((2, exp.frames + 2), SENTINEL, dtype=torch.int32, device="cuda") for _, _, exp, _ in part]
        outputs = [(t[0, 1:].data_ptr(), t[1, 1:].data_ptr()) for t in tensors]  # (a mono item gets a right array too: it must stay as it is)
        got = dec.salvage_batch_device([lac for _, lac, _, _ in part], outputs)
        torch.cuda.synchronize()
        for (name, lac, exp, status), t, (info, res, faults) in zip(part, tensors, got):
            host = t.cpu().numpy()
            _check_faults(name, lac, faults)
            assert info.frames == exp.frames and info.channels == lac[3], name
            assert host[0, 0] == SENTINEL and host[0, -1] == SENTINEL and host[1, 0] == SENTINEL and host[1, -1] == SENTINEL, name
            right = host[1, 1:-1]
            if exp.right is None:
                assert (right == SENTINEL).all(), name
            st.check(name, lac, exp, status, _codes(res.blocks, faults), _result(res), left=host[0, 1:-1],
                     right=None if exp.right is None else right)
    dec.close()


def test_truncation_of_a_three_block_stream(gpu, oracle):
    """One three-block stream cut at each block border and inside each block, single calls and scan."""
    lac = _read(os.path.join(GOLDEN, "decode_wav", "st16_lr_3blk.lac"))
    cuts = list(st.truncations(lac))
    st.cleared("gpu-three", [t for _, t in cuts])
    dec = gpu.lacx.Decoder(device=0)
    whole = dec.decode_wav(lac)
    bps = lac[3] * lac[8] // 8
    for par, t in cuts:
        info, present, flags = gpu.lacx.stream_scan(t)
        exp = st.expected(oracle, t)
        assert (present, flags, info.frames) == (exp.present, st.TRUNCATED, exp.frames), par
        image, res, faults = dec.salvage_wav(t)
        st.check(par, t, exp, None, _codes(res.blocks, faults), _result(res))
        kept = int(sum(_frames(lac)[:present]))
        assert image[:44 + kept * bps] == whole[:44 + kept * bps] and not any(image[44 + kept * bps:]), par
        assert [f.code for f in faults] == [10] * (3 - present) and res.first_bad == present
    dec.close()


def test_a_refused_container_fails_alone(gpu):
    """Inside a batch, an item whose table is refused keeps the strict parser's code and message; its neighbours -- one
    clean, one cut -- are salvaged."""
    lac = _read(os.path.join(GOLDEN, "decode_wav", "st16_lr_3blk.lac"))
    bad_table = lac[:14] + struct.pack(">I", 20000) + lac[18:]  # a block of more than 16384 frames
    assert gpu.lacx.stream_parse(bad_table) is None
    strict = gpu.lacx.lib().lacx_decode_last_error().decode()
    assert strict == "[decode-error] invalid block size"
    st.cleared("gpu-refused", [lac, bad_table, lac[:-7], lac[:20]])
    dec = gpu.lacx.Decoder(device=0)
    with pytest.raises(gpu.lacx.BatchDecodeError) as err:
        dec.salvage_wav_batch([lac, bad_table, lac[:-7], lac[:20]])
    e = err.value
    assert e.errors == {1: strict, 3: "[decode-error] truncated block size table"} and str(e) == "stream 1: " + strict
    assert e.results[1] is None and e.results[3] is None
    assert e.results[0][0] == dec.decode_wav(lac) and e.results[0][2] == []
    assert [f.code for f in e.results[2][2]] == [10] and e.results[2][1].flags == st.TRUNCATED
    with pytest.raises(RuntimeError) as one:
        dec.salvage_wav(bad_table)
    assert str(one.value) == strict  # a batch of one: no "stream 0: "
    with pytest.raises(ValueError):
        dec.salvage_wav_batch([])
    dec.close()


def test_the_strict_path_is_unchanged(gpu, selection):
    """The same damaged streams through decode_wav still raise the strict message for their lowest failing block, or
    the parser's for a cut file."""
    dec = gpu.lacx.Decoder(device=0)
    checked = 0
    for name, lac, exp, status in selection[:200]:
        if not any(exp.lost):
            continue
        if exp.flags:  # the strict parser's two rules on the payload's length, in its order
            stated = sum(s for _, s in lacmutate.table(lac)[1])
            want = "[decode-error] compressed block sizes exceed frame payload" if stated > len(lac) else "[decode-error] block payloads do not fill the file"
        else:
            b = int(np.flatnonzero(status)[0])
            want = "[decode-error] block=%d %s" % (b, TEXT[int(status[b])])
        with pytest.raises(RuntimeError) as err:
            dec.decode_wav(lac)
        assert str(err.value) == want, name
        checked += 1
    dec.close()
    assert checked >= 50


def test_cli_salvage(gpu, oracle, tmp_path):
    """`lacx_cli decode --salvage` on a damaged file and on a clean one: exit status, stderr lines, file bytes; and without
    the flag nothing changes."""
    subprocess.check_call(["make", "-C", PKG_DIR, "lacx_cli"], stdout=subprocess.DEVNULL)
    cli = os.path.join(PKG_DIR, "lacx_cli")
    lac = _read(os.path.join(GOLDEN, "decode_wav", "st16_lr_3blk.lac"))
    ent, pays = lacmutate._payloads(lac)
    pays[1] = pays[1][:1] + bytes([0x7F]) + pays[1][2:] if lac[4] == 2 else bytes([0x7F]) + pays[1][1:]
    damaged = lacmutate._rebuild(lac, ent, pays)[:-5]  # the middle block broken, the last one cut
    st.cleared("gpu-cli", [damaged])
    exp = st.expected(oracle, damaged)
    assert exp.lost == [False, True, True]
    status = dectwin.decode(lacmutate._rebuild(lac, ent, pays)).status
    (tmp_path / "bad.lac").write_bytes(damaged)
    (tmp_path / "good.lac").write_bytes(lac)
    run = lambda *a: subprocess.run([cli, *a], capture_output=True, text=True, timeout=120)  # noqa: E731
    done = run("decode", str(tmp_path / "bad.lac"), str(tmp_path / "bad.wav"), "--salvage")
    assert done.returncode == EXIT_LOSS, done.stderr
    frames = _frames(lac)
    lines = done.stderr.splitlines()
    assert lines[0] == "[salvage] block=1 frames=%d..%d %s" % (frames[0], frames[0] + frames[1] - 1, TEXT[int(status[1])])
    assert lines[1] == "[salvage] block=2 frames=%d..%d payload missing" % (frames[0] + frames[1], sum(frames) - 1)
    assert lines[2].startswith("[salvage] lost 2 of 3 blocks, %d of %d frames" % (frames[1] + frames[2], sum(frames))) and "truncated" in lines[2]
    assert (tmp_path / "bad.wav").read_bytes() == st.wav_image(exp, damaged)
    done = run("decode", str(tmp_path / "good.lac"), str(tmp_path / "good.wav"), "--salvage")
    assert done.returncode == 0 and done.stderr.splitlines() == ["[salvage] lost 0 of 3 blocks, 0 of %d frames" % sum(frames)]
    assert (tmp_path / "good.wav").read_bytes() == gpu.lacx.Decoder(device=0).decode_wav(lac)
    done = run("decode", str(tmp_path / "bad.lac"), str(tmp_path / "strict.wav"))
    assert done.returncode == 1 and "Decode failed: [decode-error] block payloads do not fill the file" in done.stderr and not (tmp_path / "strict.wav").exists()
    usage = run("decode", str(tmp_path / "bad.lac"), str(tmp_path / "x.wav"), "--nonsense")
    assert usage.returncode == 1 and "--salvage" in usage.stderr and "3" in usage.stderr
