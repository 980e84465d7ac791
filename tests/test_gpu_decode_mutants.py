"""The corpus of damaged streams (lacmutate.py) on the MI355X, compared with the CPU twin and the oracle.

The purpose of this module is to CONFIRM REFUSALS, not to provoke anything: before a single byte string goes to the
device, the whole corpus runs through the sanitized CPU twin of the lane code (mutantjudge.cleared: AddressSanitizer +
UBSan, every buffer at exactly the device path's size, every switch setting), in this same run, and only streams shown
there to stay inside their buffers are sent.  Where the sanitizer build is unavailable the module fails; it does not go
to the device unchecked.

Then: per mutant the device's answer is the twin's -- the error text "[decode-error] block=B <status text>" with the
twin's block and status -- or the oracle's samples, through decode_wav_batch (refused and valid blocks sharing waves),
through decode_window_batch_device (the gathered payload layout) and, for version-2 mutants, through k_decode_serial."""
import numpy as np
import pytest

import __graft_entry__ as ge
import lacgrammar as g
import lacmutate
import mutantjudge
import wavutil

pytestmark = pytest.mark.gpu
BATCH = 400


@pytest.fixture(scope="module")
def gpu():
    pkg = ge.load_pkg()
    if pkg.lacx.device_count() <= 0:
        pytest.fail("no HIP device: the decoder has no CPU fallback")
    return pkg


@pytest.fixture(scope="module")
def records(gpu, oracle):
    return mutantjudge.cleared(oracle, gpu.lacx.stream_parse)  # CPU first: nothing below runs if this fails


_message = mutantjudge.message


def _rate(lac):
    return (lac[5] << 8) | lac[6] | (lac[7] << 16)


def _interleaved(records):
    """Round-robin over the bases, so that neighbouring lanes hold blocks of different streams."""
    by_base = {}
    for r in records:
        by_base.setdefault(r.mutant.base, []).append(r)
    lists, out = list(by_base.values()), []
    for i in range(max(len(v) for v in lists)):
        out += [v[i] for v in lists if i < len(v)]
    return out


def test_wav_batches(gpu, oracle, records):
    """Every version-3 mutant through decode_wav_batch, a few hundred items per job, every eighth item its valid base."""
    todo = _interleaved([r for r in records if r.mutant.lac[2] == 3])
    bases = lacmutate.bases(oracle.channel_block_end)
    base_pcm = {lac: oracle.decode_ex(lac)[:2] for lac in bases.values()}
    dec = gpu.lacx.Decoder()
    checked = refused = 0
    for at in range(0, len(todo), BATCH):
        items = []  # (record or None for a base, stream)
        for i, r in enumerate(todo[at:at + BATCH]):
            items.append((r, r.mutant.lac))
            if i % 8 == 7:
                items.append((None, bases[r.mutant.base]))
        try:
            images, errors = dec.decode_wav_batch([lac for _, lac in items]), {}
        except gpu.lacx.BatchDecodeError as e:
            images, errors = e.results, e.errors
        for i, (r, lac) in enumerate(items):
            if r is None:  # a valid neighbour decodes to its base
                left, right = base_pcm[lac]
                assert i not in errors and images[i] == wavutil.make_wav(left, right, _rate(lac), lac[8]), (at, i)
            elif r.code:
                assert errors.get(i) == _message(r), (r.mutant.name, errors.get(i))
                refused += 1
            else:
                assert i not in errors, (r.mutant.name, errors[i])
                assert images[i] == wavutil.make_wav(r.left, r.right, _rate(lac), lac[8]), r.mutant.name
            checked += 1
    dec.close()
    print("wav batches: %d items, %d refused" % (checked, refused))
    assert refused > 10000


def _window_items(oracle, records):
    """(name, stream, start, frames, expected): expected = (left, right) of the window, or the error text."""
    bases = lacmutate.bases(oracle.channel_block_end)
    items = []
    for r in _interleaved([r for r in records if r.mutant.lac[2] == 3]):
        lac = r.mutant.lac
        _, ent, _ = lacmutate.table(lac)
        if len(ent) < 2:
            continue
        edges = np.concatenate([[0], np.cumsum([n for n, _ in ent])])
        if r.accepted and r.code == 0:
            seam = int(edges[len(ent) // 2])
            a, n = max(0, seam - 50), min(120, int(edges[-1]) - max(0, seam - 50))
            items.append((r.mutant.name, lac, a, n, (r.left[a:a + n], None if r.right is None else r.right[a:a + n])))
            continue
        if r.code == 0:
            continue
        b = r.block
        items.append((r.mutant.name, lac, int(edges[b]), min(64, ent[b][0]), _message(r)))
        bl, br = mutantjudge.base_pcm(oracle, r.mutant.base, bases[r.mutant.base])
        for c in lacmutate.unchanged_blocks(bases[r.mutant.base], lac):
            if r.status[c] == 0:
                a, n = int(edges[c]) + min(1, ent[c][0] - 1), min(100, ent[c][0] - min(1, ent[c][0] - 1))
                items.append((r.mutant.name, lac, a, n, (bl[a:a + n], None if br is None else br[a:a + n])))
                break
    return items


def test_window_batches(gpu, oracle, records):
    """Multi-block mutants through decode_window_batch_device: a window inside an untouched block succeeds with the
    base's (= the oracle's) frames, a window over the block the twin refuses reports that block; accepted mutants give the
    oracle's frames across a block seam.  int32 and float32.  The payload ranges of the items lie gathered back to back."""
    import torch

    items = _window_items(oracle, records)
    assert len(items) > 3000
    dec = gpu.lacx.Decoder()
    good = bad = 0
    for dtype, tdt in (("int32", torch.int32), ("float32", torch.float32)):
        for at in range(0, len(items), BATCH):
            chunk = items[at:at + BATCH]
            out = torch.zeros((len(chunk), 2, 128), dtype=tdt, device="cuda")
            ptrs = [(out[i, 0].data_ptr(), out[i, 1].data_ptr() if lac[3] == 2 else None) for i, (_, lac, _, _, _) in enumerate(chunk)]
            try:
                dec.decode_window_batch_device([x[1] for x in chunk], [x[2] for x in chunk], [x[3] for x in chunk], ptrs, dtype=dtype)
                errors = {}
            except gpu.lacx.BatchDecodeError as e:
                errors = e.errors
            torch.cuda.synchronize()
            host = out.cpu().numpy()
            for i, (name, lac, a, n, want) in enumerate(chunk):
                if isinstance(want, str):
                    assert errors.get(i) == want, (name, a, n, errors.get(i))
                    bad += 1
                    continue
                assert i not in errors, (name, a, n, errors[i])
                scale = 1.0 if dtype == "int32" else 2.0 ** -(lac[8] - 1)
                assert np.array_equal(host[i, 0, :n], (want[0] * scale).astype(host.dtype)), (name, a, n)
                if want[1] is not None:
                    assert np.array_equal(host[i, 1, :n], (want[1] * scale).astype(host.dtype)), (name, a, n)
                good += 1
    dec.close()
    print("window batches: %d windows decoded, %d refused" % (good, bad))
    assert good > 1000 and bad > 1000


def test_version_2_mutants(gpu, records):
    """The version-2 mutants through lacx.decode (k_decode_serial): the twin's block and status, or the oracle's samples."""
    todo = [r for r in records if r.mutant.lac[2] == 2]
    assert len(todo) > 500
    refused = 0
    for r in todo:
        if r.code:
            with pytest.raises(RuntimeError) as err:
                gpu.lacx.decode(r.mutant.lac)
            assert str(err.value) == _message(r), (r.mutant.name, str(err.value))
            refused += 1
        else:
            left, right, info, _ = gpu.lacx.decode(r.mutant.lac)
            assert info.version == 2 and np.array_equal(left, r.left), r.mutant.name
            assert (right is None) == (r.right is None) and (right is None or np.array_equal(right, r.right)), r.mutant.name
    assert 50 < refused < len(todo) - 50
