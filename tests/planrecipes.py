"""Input recipes of the plan-record tests (tests/test_gpu_plan_records.py) and the conditions their oracle records must
meet before a device is asked anything.  Plain helper module: integer numpy and the synth package only, so the recipes
and their conditions also run where there is no GPU (tests/test_plan_records_host.py)."""
from __future__ import annotations

import functools
import hashlib

import numpy as np

import planref

BLOCK = planref.BLOCK
PROBE = planref.PROBE
RATE = 48000


def _pkg():
    import __graft_entry__ as ge

    return ge.load_pkg()


class _MemoOracle:
    """The oracle with its per-slot answers remembered by content: the streams of the cases share blocks (the two full
    blocks in front of every final block, a stream analysed in several modes)."""

    def __init__(self):
        import oracleshim

        self._o = oracleshim
        self._memo = {}
        self.stereo_estimate = oracleshim.stereo_estimate

    def _get(self, fn, x, zr, pt):
        x = np.ascontiguousarray(x, dtype=np.int32)
        key = (fn.__name__, hashlib.blake2b(x.tobytes(), digest_size=16).digest(), x.size, bool(zr), bool(pt))
        if key not in self._memo:
            self._memo[key] = fn(x, zr, pt)
        return self._memo[key]

    def block_plan(self, x, zr=True, pt=True):
        return self._get(self._o.block_plan, x, zr, pt)

    def block_encode(self, x, zr=True, pt=True):
        return self._get(self._o.block_encode, x, zr, pt)


@functools.lru_cache(maxsize=None)
def _oracle():
    return _MemoOracle()


def windows(n):
    return [planref.slot_window(n, 4 * w)[0] for w in (1, 2, 3)]


def noise(frames, bits, seed):
    left, right = _pkg().synth.synth_pcm(frames, 2, bits, RATE, seed=seed, kind="noise", stereo="independent")
    return left.copy(), right.copy()


# -- a. probe slots over every kind of window ---------------------------------------------------------------------------

def fir_window(bits, seed):
    """256 frames that the 2-tap FIR predictor (type 1) wins: the recursion x[i] = (3 x[i-1] - x[i-2]) >> 2 that the
    predictor undoes exactly (the material of the reference's predictor selection test, restated), kept alive by a
    full-scale kick every 32 frames, so that neither a fixed order nor a quantised LPC fit gets as close."""
    full = (1 << (bits - 1)) - 1
    h = _pkg().synth._hash64(np.arange(PROBE, dtype=np.uint64), seed)
    x = np.zeros(PROBE, dtype=np.int64)
    x[0], x[1] = full * 3 // 4, full * 5 // 8
    for i in range(2, PROBE):
        x[i] = (3 * x[i - 1] - x[i - 2]) >> 2
        if i % 32 == 0:
            x[i] = (int(h[i] >> np.uint64(40)) % full) - full // 2
    return np.clip(x, -full - 1, full).astype(np.int32)


@functools.lru_cache(maxsize=None)
def stream_a(bits):
    """54 blocks of independent stereo noise (seed 3); into the three probe windows of block b the same frames of a stream
    of kind b // 6 and stereo family b % 6 (seed 100 + b), shifted right by (b % 5) * (bits // 6) bits.  Two more blocks
    whose windows carry FIR material (fir_window) in the left channel / in both, the only windows where predictor type 1
    wins."""
    synth = _pkg().synth
    nb = len(synth.KINDS) * len(synth.STEREO)
    left, right = noise((nb + 2) * BLOCK, bits, 3)
    for b in range(nb):
        kind, fam = synth.KINDS[b // len(synth.STEREO)], synth.STEREO[b % len(synth.STEREO)]
        l2, r2 = synth.synth_pcm(BLOCK, 2, bits, RATE, seed=100 + b, kind=kind, stereo=fam, start=b * BLOCK)
        sh = (b % 5) * (bits // 6)
        for w in windows(BLOCK):
            sel = slice(b * BLOCK + w, b * BLOCK + w + PROBE)
            left[sel] = l2[w:w + PROBE] >> sh
            right[sel] = r2[w:w + PROBE] >> sh
    for i, w in enumerate(windows(BLOCK)):
        a = nb * BLOCK + w
        left[a:a + PROBE] = fir_window(bits, 200 + i)
        a += BLOCK
        left[a:a + PROBE] = fir_window(bits, 210 + i) >> 1
        right[a:a + PROBE] = fir_window(bits, 220 + i) >> 2
    return left, right


def check_coverage_a(expected, bits):
    """The material does what it is here for, by the oracle's records alone."""
    assert all(b.uncertain and b.margin is not None for b in expected), \
        [i for i, b in enumerate(expected) if not (b.uncertain and b.margin is not None)]
    probes = [r for b in expected for s, r in b.slots.items() if s >= 4]
    assert len(probes) == 12 * len(expected)
    types = {r.predictor_type for r in probes}
    assert {0, 1, 2} <= types, types
    fixed = {r.order for r in probes if r.predictor_type == 0}
    assert {0, 1, 2, 3, 4} <= fixed, fixed
    lpc = {r.order for r in probes if r.predictor_type == 2}
    assert {4, 6, 8, 10, 12} <= lpc, lpc
    assert {0, 1, 2, 3} <= {r.partition_order for r in probes}
    modes = {v >> 5 for r in probes for v in r.part_mode_k}
    assert ({1, 2, 3} if bits == 16 else {0, 1, 2, 3}) <= modes, modes
    margins = [b.margin for b in expected]
    assert 0 in margins, margins          # a tie: left/right stays (mid/side only when strictly smaller)
    assert max(abs(m) for m in margins) >= 1000 and min(abs(m) for m in margins if m) <= 8, margins


# -- b. the two slots of a wave differ as much as they can --------------------------------------------------------------

PATTERNS_B = ("zeros", "constant", "alternating", "single", "last")
ROLES_B = ("L", "R", "S", "M")


def _pattern(name, amp, w):
    p = np.zeros(PROBE, dtype=np.int64)
    if name == "constant":
        p[:] = -1234
    elif name == "alternating":
        p[:] = np.where(np.arange(PROBE) % 2 == 0, amp, -amp - 1)
    elif name == "single":
        p[(0, 100, 254)[w]] = (1, -1, 1)[w]
    elif name == "last":
        p[255] = (1, -1, amp)[w]
    return p


@functools.lru_cache(maxsize=None)
def stream_b(bits):
    """One block per (pattern, role), background independent noise (seed 11).  Inside each probe window the channel `role`
    is the pattern and its partner in the slot pair is noise: role L: left = pattern, right = noise (the pair L/R);
    R: the other way round; S: right = left - pattern, so side is the pattern next to a noisy mid (the pair M/S, the
    noise at half scale so that right stays in range); M: right = pattern * 2 - left, so mid is the pattern next to a
    noisy side."""
    full = (1 << (bits - 1)) - 1
    nb = len(PATTERNS_B) * len(ROLES_B)
    left, right = noise(nb * BLOCK, bits, 11)
    for b in range(nb):
        name, role = PATTERNS_B[b // len(ROLES_B)], ROLES_B[b % len(ROLES_B)]
        for wi, w in enumerate(windows(BLOCK)):
            sel = slice(b * BLOCK + w, b * BLOCK + w + PROBE)
            if role == "L":
                left[sel] = _pattern(name, full, wi)
            elif role == "R":
                right[sel] = _pattern(name, full, wi)
            else:
                half = left[sel].astype(np.int64) >> 2
                p = _pattern(name, full >> 2, wi)
                left[sel] = half
                right[sel] = half - p if role == "S" else 2 * p - half
    lo, hi = -full - 1, full
    assert left.min() >= lo and left.max() <= hi and right.min() >= lo and right.max() <= hi
    return left, right


def check_coverage_b(expected):
    assert all(b.uncertain and b.margin is not None for b in expected), [b.uncertain for b in expected]
    # in every block at least one slot pair whose halves end far apart: one record a few bytes, its partner hundreds
    # (full-scale alternation is as expensive as noise: there the point is the magnitude, not the early end)
    for i, b in enumerate(expected):
        if PATTERNS_B[i // len(ROLES_B)] == "alternating":
            continue
        ratios = [max(b.slots[s].payload_bytes, b.slots[s + 1].payload_bytes) /
                  min(b.slots[s].payload_bytes, b.slots[s + 1].payload_bytes) for s in range(4, 16, 2)]
        assert max(ratios) >= 4, (i, ratios)


# -- c. final blocks ----------------------------------------------------------------------------------------------------

FINAL_FRAMES = (1, 2, 13, 33, 255, 256, 257, 300, 511, 512, 4095, 4096, 4097, 4098, 4351, 4352, 5000, 16383)


@functools.lru_cache(maxsize=None)
def stream_c(bits, last):
    """Two full blocks of independent noise and a final block of `last` frames.  Seed 19: by the oracle's estimate alone
    every final block of FINAL_FRAMES is uncertain at both depths (with seeds 17 and 18 the one-frame block is certain,
    and a certain block has no losers to compare)."""
    return noise(2 * BLOCK + last, bits, 19)


# -- d. the estimate's flags --------------------------------------------------------------------------------------------

SWEEP_GAINS = (0, 4, 8, 9, 10, 11, 12, 13, 14, 16, 24, 30, 31, 32, 33, 34, 40, 64)


def sweep_shifts(bits):
    return (bits // 2, bits - 6)


@functools.lru_cache(maxsize=None)
def stream_d(bits):
    """8 non-silent kinds x 6 stereo families x 4 blocks (seed 7); a gain sweep right = left * g / 32 + (noise >> j) over music,
    one block per (g, j), that walks the estimate across both of its thresholds; an all-zero block, one that is zero in the
    left channel only, one whose only non-zero sample is the last."""
    synth = _pkg().synth
    parts = []
    for kind in synth.KINDS:
        if kind == "silence":
            continue
        for fam in synth.STEREO:
            parts.append(synth.synth_pcm(4 * BLOCK, 2, bits, RATE, seed=7, kind=kind, stereo=fam))
    full = (1 << (bits - 1)) - 1
    base = synth.synth_pcm(BLOCK, 1, bits, RATE, seed=71, kind="music")[0].astype(np.int64) >> 1
    nz = noise(BLOCK, bits, 71)[1]
    for j in sweep_shifts(bits):
        for g in SWEEP_GAINS:
            r = np.clip((base * g >> 5) + (nz.astype(np.int64) >> j), -full - 1, full)
            parts.append((base.astype(np.int32), r.astype(np.int32)))
    z = np.zeros(BLOCK, dtype=np.int32)
    lastonly = z.copy()
    lastonly[-1] = 1
    parts += [(z, z), (z, nz), (z, lastonly)]
    left = np.concatenate([p[0] for p in parts]).astype(np.int32)
    right = np.concatenate([p[1] for p in parts]).astype(np.int32)
    assert left.min() >= -full - 1 and left.max() <= full and right.min() >= -full - 1 and right.max() <= full
    return left, right


GRID_BLOCKS_D = 8 * 6 * 4


def check_coverage_d(expected):
    """Each of the four classes of the estimate at least ten times in the grid; the three special blocks do what they are
    here for."""
    grid = expected[:GRID_BLOCKS_D]
    classes = {(u, m): sum(1 for b in grid if (b.uncertain, b.est_ms) == (u, m)) for u in (0, 1) for m in (0, 1)}
    assert min(classes.values()) >= 10, classes
    sweep = expected[GRID_BLOCKS_D:-3]
    assert {(b.uncertain, b.est_ms) for b in sweep} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    zero, left_zero, last_only = expected[-3:]
    assert zero.uncertain == 1 and zero.choose_ms == 0 and set(zero.slots) == {0, 1}   # the documented deviation
    assert set(left_zero.slots) <= set(range(16)) and last_only.frames == BLOCK
    return classes


@functools.lru_cache(maxsize=None)
def stream_certain(bits, nblocks):
    """`nblocks` blocks whose estimate is certain (no probe slot valid), alternately left/right and mid/side."""
    synth = _pkg().synth
    l1, r1 = synth.synth_pcm(nblocks * BLOCK, 2, bits, RATE, seed=5, kind="tone", stereo="half_silent")
    l2, r2 = synth.synth_pcm(nblocks * BLOCK, 2, bits, RATE, seed=5, kind="tone", stereo="identical")
    odd = (np.arange(nblocks * BLOCK) // BLOCK) % 2 == 1
    return np.where(odd, l2, l1).astype(np.int32), np.where(odd, r2, r1).astype(np.int32)


def check_coverage_certain(expected):
    assert all(not b.uncertain and len(b.slots) == 2 for b in expected)
    assert {b.choose_ms for b in expected} == {0, 1}


# -- expectations (cached: several tests share a stream) -----------------------------------------------------------------

_STREAMS = {"a": stream_a, "b": stream_b, "d": stream_d}


@functools.lru_cache(maxsize=None)
def expected(case, bits, mode=2, zr=True, pt=True, mono=False, arg=None, records=True):
    if case == "c":
        left, right = stream_c(bits, arg)
    elif case == "certain":
        left, right = stream_certain(bits, arg)
    else:
        left, right = _STREAMS[case](bits)
    return tuple(planref.expected_stream(_oracle(), left, None if mono else right, mode, zr, pt, records=records))
