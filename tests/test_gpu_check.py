"""Manifests honoured on the MI355X: lacx_decoder_check_batch_device and the salvage forms with a manifest per item, the
Python binding and the CLI, on streams whose damage still decodes.  Expectations come from the oracle block by block
(salvagetwin.expected) and zlib.crc32 (blockdigesttwin.judged_expectation), never from the code under test.

The purpose of this module is to CONFIRM WHAT IS FOUND, not to provoke anything: every stream below goes to the device
only after the sanitized CPU twin of the whole job (tests/native/sim_blockdigest.cpp under AddressSanitizer + UBSan, every
buffer at exactly the plan's capacity, all three forms) has passed it in this same run (blockdigesttwin.cleared).  Where
that build is unavailable the module fails; nothing goes to the device unchecked."""
import os
import random
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import blockdigesttwin as bt
import dectwin
import lacmutate
import salvagetwin as st

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PKG_DIR = os.path.join(ROOT, "lossless-audio-codec_amd")
SENTINEL = 0x5A5A5A5A
HALF = 128


@pytest.fixture(scope="module")
def gpu():
    pkg = ge.load_pkg()
    if pkg.lacx.device_count() <= 0:
        pytest.fail("no HIP device: the decoder has no CPU fallback")
    return pkg


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _frames(lac):
    return [n for n, _ in lacmutate.table(lac)[1]]


@pytest.fixture(scope="module")
def selection(gpu, oracle):
    """[(name, stream, its base's manifest, the expectation judged by it, the code-11 blocks, the plain expectation, the
    decode twin's statuses, the base's name)]: a seeded selection of at most 256 version-3 corpus mutants of small bases, half of them with
    a silently wrong block, all four length residues among those -- cleared on the CPU before any of it is used."""
    rng = random.Random("test_gpu_check")
    bases = lacmutate.bases(oracle.channel_block_end)
    small = {n for n, lac in bases.items() if lac[2] == 3 and sum(_frames(lac)) <= 40000}
    base_exp = {n: st.expected(oracle, bases[n]) for n in small}
    mans = {n: bt.manifest_for(base_exp[n], bases[n]) for n in small}
    pool = [m for m in lacmutate.corpus(oracle.channel_block_end) if m.base in small and m.lac[2] == 3]
    rng.shuffle(pool)
    hits, rest = [], []
    for m in pool:  # the oracle's word on every candidate, until both halves can be filled
        if len(hits) >= 3 * HALF and len(rest) >= HALF:
            break
        exp = st.expected(oracle, m.lac)
        exp2, wrong, collisions = bt.judged_expectation(exp, m.lac, base_exp[m.base], bases[m.base])
        assert collisions == 0
        entry = (m.name, m.lac, mans[m.base], exp2, wrong, exp, dectwin.decode(m.lac).status, m.base)
        if wrong:
            hits.append(entry)
        elif len(rest) < HALF:
            rest.append(entry)
    residue = lambda e: {_frames(e[1])[b] % 4 for b in e[4]}  # noqa: E731
    hit = [next(e for e in hits if r in residue(e)) for r in range(4)]  # one of every length residue first
    hit += [e for e in hits if not any(e is h for h in hit)][:HALF - len(hit)]
    assert len(hit) == HALF and len(rest) == HALF and set().union(*map(residue, hit)) == {0, 1, 2, 3}
    picked = hit + rest
    rng.shuffle(picked)
    bt.cleared("gpu-check", [e[1] for e in picked], [e[2] for e in picked])  # CPU first: nothing below runs if this fails
    return picked


def _codes(nb, faults):
    c = [0] * nb
    for f in faults:
        c[f.block] = f.code
    return c


def _result(r):
    return (r.blocks, r.bad_blocks, r.frames, r.lost_frames, r.first_bad, r.flags)


def test_check_batch(gpu, selection):
    """Is it intact?  Two batch calls: an item with a fault or a cut is E_MISMATCH with the lowest bad block named, its
    result and fault list as salvage fills them, code 11 exactly where the oracle's bytes differ from the base's."""
    dec = gpu.lacx.Decoder(device=0)
    found = 0
    for at in range(0, len(selection), HALF):
        part = selection[at:at + HALF]
        try:
            results, errors = dec.check_batch([e[1] for e in part], [e[2] for e in part]), {}
        except gpu.lacx.BatchDecodeError as err:
            results, errors = err.results, err.errors
        for i, ((name, lac, man, exp2, wrong, exp, status, _), got) in enumerate(zip(part, results)):
            assert got is not None, (name, errors.get(i))
            res, faults = got
            codes = _codes(res.blocks, faults)
            st.check(name, lac, exp2, status, codes, _result(res))
            assert [b for b, c in enumerate(codes) if c == bt.DIGEST] == wrong, name
            assert all(f.text == "digest mismatch" for f in faults if f.code == bt.DIGEST)
            if any(exp2.lost) or exp2.flags & st.TRUNCATED:
                first = exp2.lost.index(True)
                assert errors[i] == "[check-error] block=%d %s bad_blocks=%d" % (first, gpu.lacx.block_fault_text(codes[first]), sum(exp2.lost)), name
            else:
                assert i not in errors, (name, errors.get(i))
            found += bool(wrong)
    dec.close()
    assert found == HALF


def test_salvage_forms_with_manifests(gpu, selection):
    """The WAV form and the device form with a manifest per item, and every fifth item with none: the image and the arrays
    are the expectation's with the code-11 blocks silent; an item without a manifest is plain salvage."""
    import torch

    dec = gpu.lacx.Decoder(device=0)
    plain_with_damage = 0
    for at in range(0, len(selection), HALF):
        part = selection[at:at + HALF]
        lacs = [e[1] for e in part]
        mans = [None if i % 5 == 0 else e[2] for i, e in enumerate(part)]
        wants = [e[5] if i % 5 == 0 else e[3] for i, e in enumerate(part)]
        plain_with_damage += sum(1 for i, e in enumerate(part) if i % 5 == 0 and e[4])
        got = dec.salvage_wav_batch(lacs, manifests=mans)
        for (name, lac, _, _, _, _, status, _), want, (image, res, faults) in zip(part, wants, got):
            st.check(name, lac, want, status, _codes(res.blocks, faults), _result(res))
            assert image == st.wav_image(want, lac), name
        tensors = [torch.full((2, e[5].frames + 2), SENTINEL, dtype=torch.int32, device="cuda") for e in part]
        outputs = [(t[0, 1:].data_ptr(), t[1, 1:].data_ptr()) for t in tensors]  # rows of odd-length tensors: 4-byte aligned only
        got = dec.salvage_batch_device(lacs, outputs, manifests=mans)
        torch.cuda.synchronize()
        for (name, lac, _, _, _, _, status, _), want, t, (info, res, faults) in zip(part, wants, tensors, got):
            host = t.cpu().numpy()
            assert host[0, 0] == SENTINEL and host[0, -1] == SENTINEL and host[1, 0] == SENTINEL and host[1, -1] == SENTINEL, name
            right = host[1, 1:-1]
            if want.right is None:
                assert (right == SENTINEL).all(), name
            st.check(name, lac, want, status, _codes(res.blocks, faults), _result(res), left=host[0, 1:-1], right=None if want.right is None else right)
    dec.close()
    assert plain_with_damage >= 5  # silent damage that plain salvage hands out as good audio


def test_a_manifest_of_another_stream_and_a_refused_one(gpu, selection, oracle):
    lac, other = _read(os.path.join(GOLDEN, "decode_wav", "st16_lr_3blk.lac")), _read(os.path.join(GOLDEN, "small", "n33_mono16.lac"))
    man = bt.manifest_for(st.expected(oracle, lac), lac)
    man_other = bt.manifest_for(st.expected(oracle, other), other)
    bt.cleared("gpu-format", [lac, lac, lac, other], [man, man_other, man[:-1], man_other])
    dec = gpu.lacx.Decoder(device=0)
    with pytest.raises(gpu.lacx.BatchDecodeError) as err:
        dec.check_batch([lac, lac, lac, other], [man, man_other, man[:-1], man_other])
    e = err.value
    assert e.errors == {1: "[check-error] channels: stream 2, manifest 1", 2: "[manifest-error] size is not 32 + 8 * blocks"}
    assert str(e) == "stream 1: " + e.errors[1]
    assert e.results[1] is None and e.results[2] is None and e.results[0][1] == [] and e.results[3][1] == []
    with pytest.raises(gpu.lacx.BatchDecodeError) as err:
        dec.salvage_wav_batch([lac, lac], manifests=[man_other, man])
    assert err.value.results[0] is None and err.value.results[1][0] == dec.decode_wav(lac) and err.value.results[1][2] == []
    with pytest.raises(RuntimeError, match=r"^\[check-error\] channels: stream 2, manifest 1$"):
        dec.salvage_wav(lac, manifests=man_other)
    image, res, faults = dec.salvage_wav(lac, manifests=man)
    assert image == dec.decode_wav(lac) and faults == [] and res.bad_blocks == 0
    dec.close()


def test_handle_reuse_with_the_existing_forms_in_between(gpu, selection):
    """One decoder: check, strict decode, digest, plain salvage, check again -- every answer as on a fresh handle."""
    dec = gpu.lacx.Decoder(device=0)
    damaged = next(e for e in selection if e[4] and not any(e[5].lost))  # decodes everywhere, silently wrong somewhere
    clean = _read(os.path.join(GOLDEN, "decode_wav", "st16_lr_3blk.lac"))
    name, lac, man, exp2, wrong, exp, status, _ = damaged

    def check():
        with pytest.raises(gpu.lacx.BatchDecodeError) as err:
            dec.check_batch([lac], [man])
        res, faults = err.value.results[0]
        assert [f.block for f in faults] == wrong and all(f.code == bt.DIGEST for f in faults)
        return err.value.errors[0]

    first = check()
    wav = dec.decode_wav(clean)
    assert dec.decode_wav(lac) == st.wav_image(exp, lac)  # the strict decode hands the wrong block out: nothing refuses it
    g = dec.digest(lac)
    blocks, rows = dec.digest_blocks_batch([lac])[0]
    assert blocks.data_crc32 == g.data_crc32 and all(r.code == 0 for r in rows)
    image, res, faults = dec.salvage_wav(lac)
    assert faults == [] and image == st.wav_image(exp, lac)
    assert check() == first
    image, res, faults = dec.salvage_wav(lac, manifests=man)
    assert image == st.wav_image(exp2, lac) and [f.block for f in faults] == wrong
    assert dec.decode_wav(clean) == wav
    dec.close()


def test_cli(gpu, selection, oracle, tmp_path):
    """manifest, check, decode --salvage --manifest= and encode --manifest=: files and exit codes."""
    subprocess.check_call(["make", "-C", PKG_DIR, "lacx_cli"], stdout=subprocess.DEVNULL)
    cli = os.path.join(PKG_DIR, "lacx_cli")
    run = lambda *a: subprocess.run([cli, *a], capture_output=True, text=True, timeout=120)  # noqa: E731
    name, bad, _, exp2, wrong, exp, _, base_name = next(e for e in selection if e[4] and not any(e[5].lost) and len(e[3].lost) >= 2)
    base = lacmutate.bases(oracle.channel_block_end)[base_name]
    p = {k: str(tmp_path / k) for k in ("good.lac", "bad.lac", "good.lacm", "bad.wav", "good.wav", "src.wav", "enc.lac", "enc.lacm", "junk.lacm")}
    open(p["good.lac"], "wb").write(base)
    open(p["bad.lac"], "wb").write(bad)
    done = run("manifest", p["good.lac"], p["good.lacm"])
    assert done.returncode == 0, done.stderr
    assert _read(p["good.lacm"]) == bt.manifest_for(st.expected(oracle, base), base)
    done = run("check", p["good.lac"], p["good.lacm"])
    assert done.returncode == 0 and done.stdout.startswith("Intact: "), done.stderr
    done = run("check", p["bad.lac"], p["good.lacm"])
    frames = _frames(bad)
    edges = np.concatenate([[0], np.cumsum(frames)])
    lines = done.stderr.splitlines()
    assert done.returncode == 1, done.stderr
    assert lines[:len(wrong)] == ["[check] block=%d frames=%d..%d digest mismatch" % (b, edges[b], edges[b + 1] - 1) for b in wrong]
    open(p["junk.lacm"], "wb").write(_read(p["good.lacm"])[:-1])
    done = run("check", p["good.lac"], p["junk.lacm"])
    assert done.returncode == 2 and "[manifest-error] " in done.stderr
    done = run("decode", p["bad.lac"], p["bad.wav"], "--salvage", "--manifest=" + p["good.lacm"])
    assert done.returncode == 3, done.stderr
    lines = done.stderr.splitlines()
    assert lines[:len(wrong)] == ["[salvage] block=%d frames=%d..%d digest mismatch" % (b, edges[b], edges[b + 1] - 1) for b in wrong]
    assert _read(p["bad.wav"]) == st.wav_image(exp2, bad)
    done = run("decode", p["bad.lac"], p["good.wav"], "--salvage")  # without the manifest: handed out as good audio
    assert done.returncode == 0 and _read(p["good.wav"]) == st.wav_image(exp, bad)
    done = run("decode", p["bad.lac"], p["good.wav"], "--manifest=" + p["good.lacm"])
    assert done.returncode == 1 and "--salvage" in done.stderr
    left, right = gpu.synth.synth_pcm(16384 + 321, 2, 16, 48000, seed=5, kind="mixed")
    open(p["src.wav"], "wb").write(__import__("wavutil").make_wav(left, right, 48000, 16))
    done = run("encode", p["src.wav"], p["enc.lac"], "--verify", "--manifest=" + p["enc.lacm"])
    assert done.returncode == 0, done.stderr
    blocks = [16384, 321]
    assert _read(p["enc.lacm"]) == bt.manifest_of(2, 16, 48000, 16384 + 321, list(zip(blocks, bt.block_crcs(left, right, 16, blocks))))
    assert run("check", p["enc.lac"], p["enc.lacm"]).returncode == 0
