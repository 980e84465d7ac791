"""The stream generator of lacgrammar.py against the oracle's decoder and the reference's, with no device: proves the
generator (its Python-integer samples are what both decoders make of its bytes) and pins the oracle's decoder against the
reference's over the whole block grammar, not only over streams an encoder writes.

`ref` is refpin.reference(): the live reference where oracle/_ref exists, else the digests of
tests/golden/ref_answers.json (refusals are pinned with the reference's message)."""
import numpy as np
import pytest

import lacgrammar as g
import refpin
from refpin import same


@pytest.fixture(scope="module")
def ref():
    return refpin.reference()


@pytest.mark.parametrize("name", list(g.STATEFUL_SEQUENCES))
def test_adapt_k_restatement(oracle, ref, name):
    """Rice::adapt_k restated with plain integer division == the oracle's == the reference's, on the magnitude sequences
    the stateful cases are made of (prefix sums beyond 2^31 and 2^32, both drift directions, the flag thresholds)."""
    us = g.STATEFUL_SEQUENCES[name]
    mine = np.array(g.adapt_k_sequence(us), dtype=np.uint32)
    u = np.array(us, dtype=np.uint32)
    assert np.array_equal(mine, oracle.adapt_k_sequence(u))
    assert same(mine, ref.adapt_k_sequence(u))
    if name.startswith("large_q_") or name.startswith("zero_q_"):  # the threshold pairs differ where the flags decide
        other = {"72": "71", "71": "72", "77": "76", "76": "77"}
        twin = "_".join(other.get(w, w) for w in name.split("_"))
        assert g.adapt_k_sequence(g.STATEFUL_SEQUENCES[twin])[:len(us)] != list(mine)


def _check(name, oracle, ref):
    s = g.build(name)
    if s.ref_ok:
        want_l = np.array(s.left, dtype=np.int64)
        want_r = None if s.right is None else np.array(s.right, dtype=np.int64)
        lo, ro, ho = oracle.decode(s.lac)
        assert np.array_equal(lo, want_l) and (want_r is None) == (ro is None) and (ro is None or np.array_equal(ro, want_r))
        lr, rr, hr = ref.decode(s.lac)
        assert same(want_l.astype(np.int32), lr) and (want_r is None or same(want_r.astype(np.int32), rr))
        assert ho == hr == dict(channels=s.channels, sample_rate=s.rate, bit_depth=s.bit_depth, stereo_mode=s.stereo_mode)
        return
    with pytest.raises(RuntimeError):
        oracle.decode(s.lac)
    with pytest.raises(RuntimeError) as err:
        ref.decode(s.lac)
    # which of the reference's rules fired: the channel block's, the container's or the bit-depth check behind them
    what = {1: "invalid per-block stereo flag", 6: "channel=trailing-payload", 7: "outside PCM bit depth"}.get(s.status, "channel=primary")
    if name.startswith("beyond_2p30_q_at_limit") or name == "beyond_2p30_escape":
        what = "outside PCM bit depth"  # the token itself is accepted (see lacgrammar: the quotient limit)
    assert what in str(err.value), (name, str(err.value))


@pytest.mark.parametrize("name", list(g.CASES))
def test_directed_case(oracle, ref, name):
    _check(name, oracle, ref)


@pytest.mark.parametrize("name", list(g.WAVE_MIXES) + list(g.SWEEP))
def test_sweep_and_wave_mixes(oracle, ref, name):
    assert g.build(name).ref_ok and g.build(name).status == 0  # valid by construction, every magnitude below 2^30
    _check(name, oracle, ref)


def test_case_table_rules():
    """Status 9 only for values >= 2^30 and only in `beyond_2p30_*` cases (build() asserts both); the sweep holds several
    hundred blocks; every wave mix has at least 64 blocks of 256..1024 frames."""
    beyond = [n for n in g.CASES if n.startswith("beyond_2p30_")]
    assert all(g.build(n).status == 9 and g.build(n).max_u >= 1 << 30 for n in beyond)
    assert all(g.build(n).status != 9 for n in g.CASES if n not in beyond)
    assert sum(len(g.build(n).frames) for n in g.SWEEP) >= 300
    for n in g.WAVE_MIXES:
        fr = g.build(n).frames
        assert len(fr) >= 64 and all(256 <= f <= 1024 for f in fr)
