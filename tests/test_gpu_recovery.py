"""Recovery data on the MI355X: sidecars built, damage located and files repaired by k_recovery.hip, through the C ABI,
the Python binding and the CLI.  Expectations come from recoverytwin (log / exp tables, zlib.crc32, struct) and from the
CPU twin where the issue is the twin's bytes, never from the code under test.

The purpose of this module is to CONFIRM WHAT IS FOUND, not to provoke anything: every job below goes to the device only
after the sanitized CPU twin of the same job (tests/native/sim_recovery.cpp under AddressSanitizer + UBSan, every buffer at
exactly the plan's capacity) has passed it in this same run (recoverytwin.cleared).  Where that build is unavailable the
module fails; nothing goes to the device unchecked."""
import glob
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as ge
import blockdigesttwin as bt
import lacmutate
import recoverytwin as rt
import salvagetwin as st

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PKG_DIR = os.path.join(ROOT, "lossless-audio-codec_amd")
# per base of the corpus, in turn: small sets lose a cut-off tail, (64, 1, 1) mirrors every slice
CORPUS_SETS = [(64, 2, 4), (80, 3, 5), (256, 4, 16), (64, 1, 1), (64, 32, 224)]


def _read(path):
    with open(path, "rb") as f:
        return f.read()


FIXTURES = {os.path.basename(p)[:-4]: _read(p) for d in ("small", "decode_wav") for p in sorted(glob.glob(os.path.join(GOLDEN, d, "*.lac")))}
NAMES = sorted(FIXTURES)


@pytest.fixture(scope="module")
def gpu():
    pkg = ge.load_pkg()
    if pkg.lacx.device_count() <= 0:
        pytest.fail("no HIP device: the recovery data has no CPU fallback")
    return pkg


def _result(r):
    return (r.file_bytes, r.slices, r.bad_slices, r.repaired_slices, r.first_bad, r.parity_slices, r.bad_parity, r.worst_group,
            r.worst_group_bad, r.worst_group_parity, r.flags)


def _repair(dec, lacx, files, sides, best_effort=False):
    """(results, errors) of a repair batch, failed items included."""
    try:
        return dec.repair_batch(files, sides, best_effort), {}
    except lacx.BatchDecodeError as e:
        return e.results, e.errors


def _check(name, got, error, want):
    """One item of a repair or scan batch against the twin's Outcome."""
    if want.code == rt.INVALID:
        assert got is None and error == want.message, name
        return
    if len(got) == 3:
        data, res, bad = got
        assert data == want.out, name
    else:
        res, bad = got
    assert (_result(res), bad) == (want.result, want.bad), name
    assert (error or "") == want.message, name


def corpus_selection(block_end):
    """[(name, mutant, its base's sidecar, the twin's Outcome, the base's name)]: a seeded selection of at most 256 corpus
    mutants of small version-3 bases against their base's sidecar, the parameter set chosen per base."""
    rng = random.Random("test_gpu_recovery")
    bases = lacmutate.bases(block_end)
    small = sorted(n for n, lac in bases.items() if lac[2] == 3 and len(lac) <= 48000)
    sets = {n: CORPUS_SETS[i % len(CORPUS_SETS)] for i, n in enumerate(small)}
    sides = {n: rt.build(bases[n], *sets[n]) for n in small}
    pool = [m for m in lacmutate.corpus(block_end) if m.base in sides and m.lac[2] == 3 and m.lac != bases[m.base]]
    rng.shuffle(pool)
    fixed, refused = [], []
    for m in pool:
        if len(fixed) >= 208 and len(refused) >= 48:
            break
        want = rt.repair(m.lac, sides[m.base])
        entry = (m.name, m.lac, sides[m.base], want, m.base)
        if want.code == rt.OK and len(fixed) < 208:
            assert want.out == bases[m.base]
            fixed.append(entry)
        elif want.code == rt.MISMATCH and len(refused) < 48:
            refused.append(entry)
    picked = fixed + refused
    rng.shuffle(picked)
    return picked


@pytest.fixture(scope="module")
def selection(gpu, oracle):
    picked = corpus_selection(oracle.channel_block_end)
    # from the twin's verdicts: both kinds occur
    assert len(picked) <= 256 and sum(e[3].code == rt.OK for e in picked) >= 64 and sum(e[3].code == rt.MISMATCH for e in picked) >= 16
    for at in range(0, len(picked), 64):  # CPU first: nothing below runs if this fails
        part = picked[at:at + 64]
        files, sides = [e[1] for e in part], [e[2] for e in part]
        rt.cleared("corpus %d" % at, [rt.repair_case(files, sides), rt.repair_case(files, sides, best_effort=True), rt.repair_case(files, sides, scan_only=True)])
    return picked


@pytest.mark.parametrize("S,r,K", rt.SETS)
def test_build_equals_the_twin(gpu, S, r, K):
    """Every golden stream, 35 to 71 681 bytes (a single short slice, k < G * K, uneven groups), as one batch."""
    files = [FIXTURES[n] for n in NAMES]
    case = rt.build_case(files, S, r, K)
    twin = rt.outcomes(case, rt.cleared("build %d %d %d" % (S, r, K), [case, rt.build_case([files[3]], S, r, K)])[0])
    dec = gpu.lacx.Decoder(device=0)
    got = dec.recovery_build_batch(files, S, r, K)
    for name, data, side, want in zip(NAMES, files, got, twin):
        assert want.code == rt.OK and side == want.out, name
        info = gpu.lacx.recovery_parse(side)
        geo = rt.geometry(len(data), S, r, K)
        assert (info.file_bytes, info.slices, info.groups, info.parity_present, info.flags) == (len(data), geo.k, geo.G, geo.G * r, 0)
    if (S, r, K) == (256, 4, 16):
        assert got[NAMES.index("n16421_st16")] == rt.build(FIXTURES["n16421_st16"], S, r, K)  # and the restatement's
    assert dec.recovery(files[3], S, r, K) == got[3]
    dec.close()


def _damage(data, S, slices):
    b = bytearray(data)
    for s in slices:
        b[min(s * S + (11 * s) % S, len(b) - 1)] ^= 0xA5
    return bytes(b)


@pytest.mark.parametrize("S,r,K", rt.SETS)
def test_scan_reports_exactly_the_damaged_slices(gpu, S, r, K):
    rng = random.Random(S * 1000 + r)
    files, sides, hurt = [], [], []
    for name in NAMES:
        data = FIXTURES[name]
        geo = rt.geometry(len(data), S, r, K)
        lost = sorted(rng.sample(range(geo.k), min(geo.k, rng.choice([0, 1, 2, r, r * geo.G, r * geo.G + 1]))))
        files.append(_damage(data, S, lost))
        sides.append(rt.build(data, S, r, K))
        hurt.append(lost)
    want = [rt.scan(f, s) for f, s in zip(files, sides)]
    assert [w.bad for w in want] == hurt
    rt.cleared("scan %d %d %d" % (S, r, K), [rt.repair_case(files, sides, scan_only=True)])
    dec = gpu.lacx.Decoder(device=0)
    try:
        got, errors = dec.recovery_scan_batch(files, sides), {}
    except gpu.lacx.BatchDecodeError as e:
        got, errors = e.results, e.errors
    for i, name in enumerate(NAMES):
        _check(name, got[i], errors.get(i), want[i])
    dec.close()


def test_corpus_repair(gpu, selection):
    """Mutants of the corpus against their base's sidecar: the twin's verdict per item -- the base's bytes back, or the
    refusal naming the lowest group beyond its parity."""
    dec = gpu.lacx.Decoder(device=0)
    fixed = 0
    for at in range(0, len(selection), 64):
        part = selection[at:at + 64]
        got, errors = _repair(dec, gpu.lacx, [e[1] for e in part], [e[2] for e in part])
        for i, (name, lac, side, want, base) in enumerate(part):
            _check(name, got[i], errors.get(i), want)
            fixed += want.code == rt.OK and got[i][0] is not None
    dec.close()
    assert fixed >= 64


def test_refusals_and_best_effort_equal_the_twin(gpu, selection):
    dec = gpu.lacx.Decoder(device=0)
    refused = [e for e in selection if e[3].code == rt.MISMATCH]
    files, sides = [e[1] for e in refused], [e[2] for e in refused]
    want = [rt.repair(f, s, best_effort=True) for f, s in zip(files, sides)]
    rt.cleared("refused", [rt.repair_case(files, sides, best_effort=True), rt.repair_case(files, sides)])
    got, errors = _repair(dec, gpu.lacx, files, sides, best_effort=True)
    for i, e in enumerate(refused):
        assert want[i].code == rt.MISMATCH and want[i].out is not None and want[i].result[10] & rt.UNREPAIRED
        _check(e[0], got[i], errors.get(i), want[i])
        assert errors[i].startswith("[recovery-error] group ")
    got, errors = _repair(dec, gpu.lacx, files, sides)
    for i, e in enumerate(refused):
        assert got[i][0] is None
        _check(e[0], got[i], errors.get(i), e[3])
    dec.close()


def test_a_repaired_stream_passes_its_manifest(gpu, selection, oracle):
    """After a repair, check with the manifest confirms it: the repaired bytes decode block by block to what the base's
    manifest says, while the damaged ones did not all."""
    bases = lacmutate.bases(oracle.channel_block_end)
    part = [e for e in selection if e[3].code == rt.OK][:32]
    mans = {}
    for e in part:
        if e[4] not in mans:
            mans[e[4]] = bt.manifest_for(st.expected(oracle, bases[e[4]]), bases[e[4]])
    rt.cleared("recovery-manifest repair", [rt.repair_case([e[1] for e in part], [e[2] for e in part])])
    dec = gpu.lacx.Decoder(device=0)
    got, errors = _repair(dec, gpu.lacx, [e[1] for e in part], [e[2] for e in part])
    assert not errors
    repaired = [g[0] for g in got]
    bt.cleared("recovery-manifest", repaired, [mans[e[4]] for e in part])
    for (res, faults), e in zip(dec.check_batch(repaired, [mans[e[4]] for e in part]), part):
        assert faults == [] and res.bad_blocks == 0, e[0]
    dec.close()


def test_one_batch_keeps_per_item_outcomes(gpu):
    """Intact, repairable, unrepairable, refused sidecar, short sidecar, truncated file: one batch, each item its own answer;
    then the same decoder builds, decodes and repairs again."""
    S, r, K = 256, 4, 16
    a, b = FIXTURES["n16421_st16"], FIXTURES["n4097_st16"]
    sa, sb = rt.build(a, S, r, K), rt.build(b, 80, 3, 5)
    geo = rt.geometry(len(a), S, r, K)
    files = [a, _damage(a, S, range(5, 5 + r * geo.G)), _damage(a, S, rt.members(geo, 2)[:r + 1]), a, _damage(a, S, [0, 1]), a[:len(a) - 3 * S - 7], _damage(b, 80, [1, 100]), b""]
    sides = [sa, sa, sa, b"LACX" + sa[4:], sa[:40 + 4 * geo.k + (S + 4) + 9], sa, sb, sb]
    for best in (False, True):
        want = [rt.repair(f, s, best) for f, s in zip(files, sides)]
        assert [w.code for w in want] == [rt.OK, rt.OK, rt.MISMATCH, rt.INVALID, rt.MISMATCH, rt.OK, rt.OK, rt.MISMATCH]
        rt.cleared("batch %d" % best, [rt.repair_case(files, sides, best), rt.build_case([a], S, r, K), rt.repair_case([files[1]], [sa]),
                                       rt.repair_case([files[2]], [sa], best)])
        dec = gpu.lacx.Decoder(device=0)
        got, errors = _repair(dec, gpu.lacx, files, sides, best)
        for i, w in enumerate(want):
            _check("item %d" % i, got[i], errors.get(i), w)
        with pytest.raises(gpu.lacx.BatchDecodeError) as err:
            dec.repair_batch(files, sides, best)
        assert str(err.value) == "stream 2: " + want[2].message
        # the handle goes on: a build, a strict decode and a repair of one
        assert dec.recovery(a, S, r, K) == sa
        assert dec.decode_wav(b) == gpu.lacx.Decoder(device=0).decode_wav(b)
        data, res, bad = dec.repair(files[1], sa)
        assert data == a and bad == list(range(5, 5 + r * geo.G)) and res.repaired_slices == r * geo.G
        with pytest.raises(RuntimeError, match=r"^\[recovery-error\] group 2: 5 damaged slices, 4 parity slices usable$"):
            dec.repair(files[2], sa, best)
        dec.close()


def test_call_level_refusals(gpu):
    dec = gpu.lacx.Decoder(device=0)
    lac = FIXTURES["n33_mono16"]
    rt.cleared("call level", [rt.build_case([lac], 64, 2, 4)])
    with pytest.raises(ValueError, match=r"^\[recovery-error\] slice_bytes 100 is not a multiple of 16 in 64\.\.65536$"):
        dec.recovery_build_batch([lac], 100, 2, 4)
    with pytest.raises(ValueError, match=r"^\[recovery-error\] group_data 255 is not in 1\.\.256 - parity$"):
        dec.recovery_build_batch([lac], 64, 2, 255)
    with pytest.raises(ValueError):
        dec.recovery_build_batch([])
    with pytest.raises(ValueError):
        dec.repair_batch([], [])
    with pytest.raises(gpu.lacx.BatchDecodeError) as err:  # not a stream: the strict parser's code and text
        dec.recovery_build_batch([lac, lac[:20], b"RIFF" + lac[4:]], 64, 2, 4)
    assert sorted(err.value.errors) == [1, 2] and err.value.results[0] == rt.build(lac, 64, 2, 4)
    for i, blob in ((1, lac[:20]), (2, b"RIFF" + lac[4:])):
        assert gpu.lacx.stream_parse(blob) is None and err.value.errors[i] == gpu.lacx.lib().lacx_decode_last_error().decode()
    with pytest.raises(ValueError, match=r"^\[recovery-error\] wrong magic$"):
        gpu.lacx.recovery_parse(b"LACM" + bytes(60))
    dec.close()


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as ge
lacx = ge.load_pkg().lacx
good, bad, side = (open(p, "rb").read() for p in sys.argv[2:5])
dec = lacx.Decoder(device=0)
assert dec.recovery(good, 256, 4, 16) == side
data, res, slices = dec.repair(bad, side)
assert data == good and res.repaired_slices == len(slices) == 3
try:
    dec.recovery_scan_batch([good, bad], [side, side])
    raise SystemExit(5)
except lacx.BatchDecodeError as e:
    assert list(e.errors) == [1] and e.results[1][1] == slices and e.results[0][1] == []
    print(e.errors[1])
"""


def test_binding_and_cli_in_a_child_process(gpu, oracle, tmp_path):
    """The Python binding in a process of its own, and lacx_cli protect / repair / encode --recovery=: files and exit codes
    (0 intact or fully repaired, 1 not fully repaired -- out.lac only with --best-effort --, 2 refused)."""
    subprocess.check_call(["make", "-C", PKG_DIR, "lacx_cli"], stdout=subprocess.DEVNULL)
    cli = os.path.join(PKG_DIR, "lacx_cli")
    run = lambda *a: subprocess.run([cli, *a], capture_output=True, text=True, timeout=120)  # noqa: E731
    S, r, K = 256, 4, 16
    good = FIXTURES["n16421_st16"]
    geo = rt.geometry(len(good), S, r, K)
    side = rt.build(good, S, r, K)
    bad = _damage(good, S, [3, 4, 90])
    worse = _damage(good, S, rt.members(geo, 1)[:r + 1] + [0])
    rt.cleared("cli", [rt.build_case([good], S, r, K), rt.build_case([good]), rt.repair_case([good], [side]), rt.repair_case([bad], [side]),
                       rt.repair_case([worse], [side]), rt.repair_case([worse], [side], best_effort=True), rt.repair_case([bad], [side], scan_only=True),
                       rt.repair_case([good, bad], [side, side], scan_only=True)])
    p = {k: str(tmp_path / k) for k in ("good.lac", "bad.lac", "worse.lac", "good.lacr", "default.lacr", "junk.lacr", "out.lac", "src.wav", "enc.lac", "enc.lacr")}
    for k, v in (("good.lac", good), ("bad.lac", bad), ("worse.lac", worse), ("junk.lacr", side[:30])):
        open(p[k], "wb").write(v)
    done = run("protect", p["good.lac"], p["good.lacr"], "--slice=256", "--parity=4", "--group=16")
    assert done.returncode == 0 and _read(p["good.lacr"]) == side, done.stderr
    done = run("protect", p["good.lac"], p["default.lacr"])
    assert done.returncode == 0 and _read(p["default.lacr"]) == rt.build(good), done.stderr
    assert run("protect", p["good.lac"], p["out.lac"], "--slice=100").returncode == 2 and not os.path.exists(p["out.lac"])
    assert run("protect", p["junk.lacr"], p["out.lac"]).returncode == 2 and not os.path.exists(p["out.lac"])
    child = subprocess.run([sys.executable, "-c", CHILD, ROOT, p["good.lac"], p["bad.lac"], p["good.lacr"]], capture_output=True, text=True, timeout=300)
    assert child.returncode == 0, child.stderr
    assert child.stdout.strip() == "[recovery-error] slice=3 bad_slices=3 repairable"
    done = run("repair", p["good.lac"], p["good.lacr"], p["out.lac"])
    assert done.returncode == 0 and done.stdout.startswith("Intact: ") and _read(p["out.lac"]) == good, done.stderr
    os.remove(p["out.lac"])
    done = run("repair", p["bad.lac"], p["good.lacr"], p["out.lac"])
    assert done.returncode == 0 and done.stdout.startswith("Repaired: 3 of 3 damaged slices") and _read(p["out.lac"]) == good, done.stderr
    os.remove(p["out.lac"])
    done = run("repair", p["worse.lac"], p["good.lacr"], p["out.lac"])
    assert done.returncode == 1 and "[recovery-error] group 1: 5 damaged slices, 4 parity slices usable" in done.stderr and not os.path.exists(p["out.lac"])
    done = run("repair", p["worse.lac"], p["good.lacr"], p["out.lac"], "--best-effort")
    assert done.returncode == 1 and _read(p["out.lac"]) == rt.repair(worse, side, best_effort=True).out, done.stderr
    assert run("repair", p["bad.lac"], p["junk.lacr"], p["out.lac"]).returncode == 2
    left, right = gpu.synth.synth_pcm(16384 + 321, 2, 16, 48000, seed=5, kind="mixed")
    rt.cleared("cli encode", [rt.build_case([oracle.encode(left, right, 48000, 16, 2)])])  # the bytes the encoder will give
    open(p["src.wav"], "wb").write(__import__("wavutil").make_wav(left, right, 48000, 16))
    done = run("encode", p["src.wav"], p["enc.lac"], "--recovery=" + p["enc.lacr"])
    assert done.returncode == 0 and _read(p["enc.lacr"]) == rt.build(_read(p["enc.lac"])), done.stderr
