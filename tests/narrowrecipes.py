"""The corpus of the streaming block tests (tests/test_narrow_blocks_host.py, tests/test_gpu_narrow_blocks.py) and the
conditions its oracle records must meet before a device is asked anything.  Plain helper module: numpy, the oracle and
lacgrammar only, no GPU, no test in here.

"Narrow" is the streaming domain, |x| <= 2^24: what `lacx_block_encode` sends to k_analyze<16,1024> with its fused emit
and the packer, and behind them k_offsets / k_emit / k_pack -- the kernels the benchmark times.

Why it exists.  A census of what the generic material reaches (the oracle's plans of L, R, M and S of one 16384-sample
block of each of the nine synth kinds at 16 and 24 bit, seed 33: 72 whole-block plans, 838 partitions):
  partition orders   1: 55 plans, 2: 6, 4: 4, 6: 4, 7: 3; orders 0, 3, 5 and 8 never
  modes              687 of 838 partitions static Rice (3); mode 0 16 times, bin (2) 21 times
  predictors         FIR never, LPC order 6 never, fixed order 3 once
  Rice parameters    4, 10, 11, 13 and everything above 15 never
So a partition border inside a thread's 16-sample chunk, a long last partition, 256 partitions of 32 samples, the
silent-chunk shortcut across chunk and partition ends, the 34-bit escape, unary runs of 32 ones and more, `run - 4`
tokens of thousands, 64-bit sums at high partition orders and Rice parameters in the twenties ran by accident or not at
all.  The families below reach them on purpose and check_coverage() asserts, on the oracle's records alone, that they do.

Everything is built from explicit seeds; seeds found by search (always: seed = 0, 1, 2, ... through the oracle, first hit
kept) are frozen as literals next to what they were chosen for; nothing searches at import time.

Left out, after bounded searches:
  * a whole block of >= 4097 samples where partition order 0 wins with partitioning on.  Order 1 is taken whenever it is
    within 5 % of the unpartitioned size (oracle/lac_oracle.c, the partition loop of laco_block_plan), and the stateful parameter differs from the
    stateless one by its +-1 bias alone.  Searched: _geometry(n, 0, seed) and _runs_material(n, seed) for seed 0..59 and
    all-zero, constant, ramp, sine, +-1 and white blocks of 3 .. 2^20, at n = 4097, 8192 and 16384: none.  The whole-block
    adaptive walk is reached with partitioning off (check_flag_coverage).
  * an LPC winner whose Levinson recursion stopped early (used < candidate order).  Inside the 25-bit domain the
    autocorrelation sums are exact, the prediction error stays >= the square of the first non-zero sample and never
    falls below the recursion's 1e-8.  Searched: _sines(seed, n) for seed 0..399 at n = 16384 and 4097, and noiseless
    sines of amplitude 1 .. 2^23: none (the wide corpus gets its early stops from sums that wrap).

The largest Rice parameter in force that the oracle gives on full-scale 24-bit side material is 26 (KMAX, measured): the
side channel S = L - R of full-scale channels of opposite, randomly changing sign jumps between +-(2^24 - 1), fixed order
1 wins, its residual has zigzag values up to 2^26 and the stateful parameter follows their mean.  The table itself holds
0..15 for a static partition and 0..12 as the start of an adaptive one; the family `parameters` reaches 0..15 in static
partitions and 12, 16..26 in force inside adaptive ones, together every value 0..26.

Flag pairs: every block runs with (zero runs on, partitioning on); the families `geometry` and `tokens` (FLAG_SUBSET)
run under the other three pairs as well.

check_coverage() + check_flag_coverage() take about 10 s on the CPU (112 blocks, 72 of them under four flag pairs, and the
Python token walk of 18 blocks); tests/test_narrow_blocks_host.py as a whole about 47 s.
"""
from __future__ import annotations

import functools

import numpy as np

import lacgrammar as G
import planref
from widerecipes import FLAGS, Block, _segment, classify, max_partition_order

EDGE = 1 << 24
FULL24, FULL16 = (1 << 23) - 1, (1 << 15) - 1
NARROW_LIMIT = (1 << 32) - (1 << 20)  # kNarrowLimit, csrc/analyze_core.h
CHUNK = 16                            # samples per thread of k_analyze<16,1024>
KMAX = 26
BLOCK = 16384

GEOMETRY_N = (4097, 8191, 8192, 8223, 12289, 16368, 16383, 16384)
TOKEN_N = (16384, 12289)
LOUD_N = (16384, 16383)
PREDICTOR_N = (16384, 4097)
FLAG_SUBSET = ("geometry", "tokens")
FAMILIES = ("geometry", "tokens", "parameters", "loud", "predictors", "stereo")


def i32(x):
    x = np.asarray(x)
    assert np.abs(x.astype(np.int64)).max(initial=0) <= EDGE
    return x.astype(np.int32)


# -- frozen results of the searches -------------------------------------------------------------------------------------

# seed of _geometry(n, p, seed): the first seed whose oracle plan has partition order p (0 everywhere but here)
GEOMETRY_SEEDS = {(4097, 2): 1, (8192, 4): 1, (12289, 2): 1, (16368, 6): 1, (16384, 2): 1}
# (n, seed of _sines(seed, n), predictor type, order)
PREDICTORS = ((16384, 39, 0, 0), (16384, 85, 0, 2), (16384, 1, 0, 3), (16384, 8, 0, 4), (16384, 18, 2, 4),
              (16384, 30, 2, 6), (16384, 55, 2, 8), (16384, 5, 2, 10), (16384, 0, 2, 12), (16384, 47, 2, 12),
              (4097, 80, 0, 0), (4097, 38, 0, 1), (4097, 114, 0, 2), (4097, 1, 0, 3), (4097, 9, 0, 4), (4097, 8, 2, 4),
              (4097, 128, 2, 6), (4097, 14, 2, 8), (4097, 21, 2, 10), (4097, 0, 2, 12))
SATURATED = ((16384, 47), (4097, 128))  # LPC winners with a Q15 coefficient at -32768 or 32767
# (n, seed of _fir(seed, n)): the 2-tap FIR predictor wins (not searched for: it does for every seed 0..19)
FIR = ((16384, 1), (4097, 1))
# seed of _loud(n, above, seed): fixed order 0 wins (so that the residual sum is the samples' own) at partition order >= 3
LOUD_SEEDS = {(16384, False): 0, (16384, True): 0, (16383, False): 0, (16383, True): 0}
WANT_PREDICTORS = {(0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (2, 4), (2, 6), (2, 8), (2, 10), (2, 12)}


# -- families -----------------------------------------------------------------------------------------------------------

def _geometry(n, p, seed):
    """2^p partitions of n >> p samples (the last one longer) whose character changes from each to the next (zeros with
    one 1, 0 / +-1 / +-2, quiet, medium and loud noise), so that order p separates what order p - 1 mixes."""
    rng = np.random.default_rng([n, p, seed])
    cycle = [("z", 0), ("b", 0), ("q", int(rng.integers(3, 9))), ("m", int(rng.integers(9, 15))),
             ("h", int(rng.integers(15, 21)))]
    cycle = [cycle[i] for i in rng.permutation(5)[:int(rng.integers(2, 5))]]
    parts, base = 1 << p, n >> p
    segs = []
    for i in range(parts):
        length = n - base * (parts - 1) if i + 1 == parts else base
        character, bits = cycle[i % len(cycle)]
        segs.append(_segment(rng, character, length, bits))
    return i32(np.concatenate(segs))


def _sparse(n, seed):
    """Zeros with a spike of up to 2^20 every 600..900 samples: zero-run partitions whose parameter sits near 0 when a
    spike comes (the 34-bit escape), run tokens of hundreds."""
    rng = np.random.default_rng([21, n, seed])
    x = np.zeros(n, dtype=np.int64)
    a = 40
    while a < n:
        x[a] = int(rng.choice([-1, 1])) * int(rng.integers(1 << 10, 1 << 20))
        a += int(rng.integers(600, 900))
    return i32(x)


def _one_partition(n, seed):
    """Zero everywhere but for a few spikes in the first hundred samples: all that is not zero lies inside the first
    partition, the run behind it is cut at every partition end and a run of thousands is one token."""
    rng = np.random.default_rng([22, n, seed])
    x = np.zeros(n, dtype=np.int64)
    x[rng.choice(100, size=6, replace=False)] = rng.integers(100, 5000, size=6)
    return i32(x)


def _runs_material(n, seed):
    """Bursts of 3..12 non-zero samples of up to +-30 between zero runs of 1..5 and of 20..60 samples: short runs on
    either side of every chunk border and across it, inside zero-run partitions."""
    rng = np.random.default_rng([23, n, seed])
    out = []
    size = 0
    while size < n:
        burst = rng.integers(1, 31, size=int(rng.integers(3, 13))) * rng.choice([-1, 1])
        run = int(rng.integers(1, 6)) if rng.random() < 0.6 else int(rng.integers(20, 61))
        out += [burst, np.zeros(run, dtype=np.int64)]
        size += burst.size + run
    return i32(np.concatenate(out)[:n])


def _outliers(n, seed):
    """Noise of +-(4..12) without a zero, an outlier about every 1500 samples, alternately of 270..480 and of 600..3000:
    static Rice partitions whose unary part runs to 32..63 ones and to hundreds."""
    rng = np.random.default_rng([24, n, seed])
    x = rng.integers(4, 13, size=n) * rng.choice([-1, 1], size=n)
    a = 700
    while a < n:
        x[a] = int(rng.choice([-1, 1])) * int(rng.integers(270, 480) if (a & 1) else rng.integers(600, 3000))
        a += int(rng.integers(1200, 1800))
    return i32(x)


def _bin_material(n, seed):
    """+-1 / +-2 with a zero at every fifth sample (no zero run), +-(3..8) at one sample in thirty and a sample of up to
    2^20 at the start of every eighth of the block: after one of those the adaptive k is of no use for the small values
    and no static k serves both, the bin code still does."""
    rng = np.random.default_rng([25, n, seed])
    x = rng.choice([-2, -1, 1, 2], size=n)
    x[::5] = 0
    at = rng.random(n) < 1 / 30
    x[at] = (rng.integers(3, 9, size=n) * rng.choice([-1, 1], size=n))[at]
    x[::n >> 3] = rng.integers(1 << 14, 1 << 20, size=x[::n >> 3].size)
    return i32(x)


def _levels(n, bits, fade, seed):
    """One partition of n / len(bits) samples per entry: noise of +-2^bits, or -- fade -- noise that grows from 2^(bits - 4)
    to 2^bits over the partition, which the adaptive parameter follows and a static one does not."""
    rng = np.random.default_rng([26, n, seed])
    base = n // len(bits)
    segs = []
    for i, b in enumerate(bits):
        length = n - base * (len(bits) - 1) if i + 1 == len(bits) else base
        amp = float(1 << b) * (2.0 ** np.linspace(-4, 0, length) if fade else np.ones(length))
        segs.append(np.rint(rng.uniform(-1, 1, size=length) * amp))
    return i32(np.concatenate(segs))


def _opposed_full_scale(n, seed):
    """(L, R) at 24-bit full scale and of opposite sign at every sample, so that S = L - R is +-(2^24 - 1)."""
    sign = np.random.default_rng([27, n, seed]).integers(0, 2, size=n).astype(bool)
    left = np.where(sign, FULL24, -FULL24 - 1)
    return left.astype(np.int32), (-left - 1).astype(np.int32)


def _loud(n, above, seed):
    """Eight stretches of noise, alternately quiet and loud, whose zigzag sum is exactly kNarrowLimit - 1 or kNarrowLimit:
    with order 0 the winner, the last block on the 32-bit paths and the first on the 64-bit ones."""
    rng = np.random.default_rng([28, n, seed])
    mean = NARROW_LIMIT / n
    segs = [rng.integers(-int(a), int(a) + 1, size=n // 8 if i < 7 else n - 7 * (n // 8))
            for i, a in enumerate([mean * 0.25, mean * 1.75] * 4)]
    x = np.concatenate(segs).astype(np.int64)
    want = NARROW_LIMIT - (0 if above else 1)
    d = want - int(_zigzag(x).sum())
    if d % 2:  # zigzag(v) = 2 v for v >= 0 and -2 v - 1 below: one sign turned makes the difference even
        at = int(np.flatnonzero(x > mean)[0])
        x[at] = -x[at]
        d += 1
    idx = np.flatnonzero(x > mean)  # the rest in equal steps over the loud positive samples
    q, r = divmod(abs(d) // 2, idx.size)
    x[idx] += (1 if d > 0 else -1) * q
    x[idx[:r]] += 1 if d > 0 else -1
    assert int(_zigzag(x).sum()) == want
    return i32(x)


def _zigzag(x):
    x = np.asarray(x, dtype=np.int64)
    return (x << 1) ^ (x >> 63)


def _sines(seed, n):
    """One or two sines of period 2.2..60 samples and amplitude 2^8..2^22.9, noise of 2^0..2^15, inside 24 bits: the
    material of the predictor search."""
    rng = np.random.default_rng([7, seed, n])
    t = np.arange(n, dtype=np.float64)
    x = np.zeros(n, dtype=np.float64)
    for _ in range(int(rng.integers(1, 3))):
        period = rng.uniform(2.2, 60.0)
        amp = 2.0 ** rng.uniform(8, 22.9)
        x += amp * np.sin(2 * np.pi * t / period + rng.uniform(0, 6.28))
    x = np.rint(x).astype(np.int64)
    nb = int(rng.integers(0, 16))
    x += rng.integers(-(1 << nb), (1 << nb) + 1, size=n)
    return i32(np.clip(x, -FULL24 - 1, FULL24))


def _fir(seed, n):
    """The recursion x[i] = (3 x[i-1] - x[i-2]) >> 2 that the FIR predictor undoes exactly, kicked every 16 samples."""
    rng = np.random.default_rng([11, seed, n])
    x = np.zeros(n, dtype=np.int64)
    x[0], x[1] = FULL24 * 3 // 4, FULL24 * 5 // 8
    for i in range(2, n):
        x[i] = (3 * x[i - 1] - x[i - 2]) >> 2
        if i % 16 == 0:
            x[i] = int(rng.integers(-FULL24 // 2, FULL24 // 2))
    return i32(np.clip(x, -FULL24 - 1, FULL24))


def _stereo_pair(bits, n, seed):
    """(L, R) = common +- d: the common part stationary noise a quarter of full scale, d 64 stretches of changing
    character far below it, so that L, R and M look stationary and S = 2 d does not; where d allows it both channels
    touch the ends of the range with opposite sign, so that |S| reaches 2^bits - 1."""
    rng = np.random.default_rng([29, bits, n, seed])
    full = (1 << (bits - 1)) - 1
    common = rng.integers(-(full >> 2), (full >> 2) + 1, size=n)
    d = np.concatenate([_segment(rng, "zbq"[i % 3], n // 64 if i < 63 else n - 63 * (n // 64), 5) for i in range(64)])
    left, right = common + d, common - d
    at = np.flatnonzero(d == 0)[::97]
    left[at] = np.where(np.arange(at.size) % 2 == 0, full, -full - 1)
    right[at] = -left[at] - 1
    return left.astype(np.int32), right.astype(np.int32)


STEREO_PAIRS = (("l24", "r24", 24), ("l16", "r16", 16), ("l24_ragged", "r24_ragged", 24))
# partition orders of (L, R, M, S) of each pair, as the oracle plans them
STEREO_ORDERS = {"l24": (1, 1, 5, 8), "l16": (1, 1, 2, 8), "l24_ragged": (1, 1, 5, 8)}

PARAMETER_BLOCKS = (  # (name, bits of the partitions, fade)
    ("static_0_to_7", (0, 7, 1, 6, 2, 5, 3, 4), False), ("static_8_to_15", (8, 15, 9, 14, 10, 13, 11, 12), False),
    ("static_16_to_23", (16, 23, 17, 22, 18, 21, 19, 20), False), ("static_24_and_low", (24, 3, 24, 12, 24, 0, 24, 19), False),
    ("fade_4_to_11", (4, 11, 5, 10, 6, 9, 7, 8), True), ("fade_12_to_19", (12, 19, 13, 18, 14, 17, 15, 16), True),
    ("fade_20_to_24", (20, 24, 21, 23, 22, 20, 24, 21), True))


@functools.lru_cache(maxsize=None)
def corpus():
    """Every block of the corpus as (family, name, samples), in a fixed order."""
    out = []
    for n in GEOMETRY_N:
        for p in range(1, max_partition_order(n) + 1):
            out.append(Block("geometry", f"n{n}_p{p}", _geometry(n, p, GEOMETRY_SEEDS.get((n, p), 0))))
    for n in TOKEN_N:
        out.append(Block("tokens", f"sparse_escapes_n{n}", _sparse(n, 0)))
        out.append(Block("tokens", f"one_partition_n{n}", _one_partition(n, 0)))
        out.append(Block("tokens", f"short_runs_n{n}", _runs_material(n, 0)))
        out.append(Block("tokens", f"outliers_n{n}", _outliers(n, 0)))
        out.append(Block("tokens", f"bin_n{n}", _bin_material(n, 0)))
    for name, bits, fade in PARAMETER_BLOCKS:
        out.append(Block("parameters", name, _levels(BLOCK, bits, fade, 0)))
    left, right = _opposed_full_scale(BLOCK, 0)
    out.append(Block("parameters", "side_of_opposed_full_scale", planref.mid_side(left, right)[1]))
    for n in LOUD_N:
        for above in (False, True):
            out.append(Block("loud", f"n{n}_{'at' if above else 'below'}_the_limit", _loud(n, above, LOUD_SEEDS[n, above])))
    for n, seed, ptype, order in PREDICTORS:
        out.append(Block("predictors", f"n{n}_seed{seed}_type{ptype}_order{order}", _sines(seed, n)))
    for n, seed in FIR:
        out.append(Block("predictors", f"n{n}_fir_seed{seed}", _fir(seed, n)))
    for (lname, rname, bits), n in zip(STEREO_PAIRS, (BLOCK, BLOCK, 12289)):
        left, right = _stereo_pair(bits, n, 0)
        out += [Block("stereo", lname, left), Block("stereo", rname, right)]
    assert len({(b.family, b.name) for b in out}) == len(out)
    for b in out:
        assert np.abs(b.x.astype(np.int64)).max() <= EDGE, (b.family, b.name)
        b.x.setflags(write=False)
    return tuple(out)


def family(name):
    return tuple(b for b in corpus() if b.family == name)


def block(family_name, name):
    return next(b for b in corpus() if (b.family, b.name) == (family_name, name))


def fits(x, bits):
    x = np.asarray(x, dtype=np.int64)
    return bool(x.min() >= -(1 << (bits - 1)) and x.max() < (1 << (bits - 1)))


def ragged_blocks():
    """The geometry and tokens blocks that are not a whole 16384 samples."""
    return tuple(b for b in corpus() if b.family in FLAG_SUBSET and b.x.size != BLOCK)


def streams():
    """((name, bit depth, left, right), ...): the 16384-sample blocks of the corpus that fit 24 bits, in corpus order,
    alternately left and right, in streams of at most 40 blocks; each stream ends with a ragged corpus block pair."""
    full = [b for b in corpus() if b.x.size == BLOCK and fits(b.x, 24) and b.family != "stereo"]
    ragged = [b for b in ragged_blocks() if fits(b.x, 24)]
    out = []
    for s, a in enumerate(range(0, len(full) - 1, 80)):
        part = full[a:a + 80]
        part = part[:len(part) & ~1]
        tail = [b for b in ragged if b.x.size == (12289, 8223, 4097)[s % 3]][:2]
        left = np.concatenate([b.x for b in part[0::2]] + [tail[0].x])
        right = np.concatenate([b.x for b in part[1::2]] + [tail[1].x])
        out.append((f"stream{s}", 24, left, right))
    return tuple(out)


def stereo_streams():
    """((name, bit depth, left, right), ...) of the stereo family: each pair as a stream of its own."""
    return tuple((l, bits, block("stereo", l).x, block("stereo", r).x) for l, r, bits in STEREO_PAIRS)


# -- the oracle's records -----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _oracle():
    import oracleshim

    oracleshim.lib()
    return oracleshim


@functools.lru_cache(maxsize=None)
def expected(family_name, zr=True, pt=True):
    """((block, slot record, oracle bytes), ...) of a family under one flag pair; computed once, shared."""
    o = _oracle()
    return tuple((b, planref.slot_record(o, b.x, zr, pt), o.block_encode(b.x, zr, pt)) for b in family(family_name))


def _modes(record):
    return {v >> 5 for v in record.part_mode_k}


def residual(x, record):
    """The zigzag residual of the record's predictor, by lacgrammar.residuals_of."""
    coef = list(record.coef) if record.predictor_type == 2 else []
    return [G.zigzag(r) for r in G.residuals_of(record.predictor_type, record.order, coef, [int(v) for v in x])]


def tokens_of(x, record):
    """The tokens of every partition, from the record and the residual alone: [(mode, k of the table, start, size,
    [(kind, position, zigzag value or run length, parameter in force), ...]), ...].  Kinds as in lacgrammar.Part:
    v (bare Rice code), n / r / e (zero-run mode: normal, run, escape), z / s / f (bin mode: zero, small, fallback)."""
    u = residual(x, record)
    p = record.partition_order
    out, start = [], 0
    for size, mk in zip(G.partition_sizes(len(u), p), record.part_mode_k):
        mode, k0 = mk >> 5, mk & 31
        us = u[start:start + size]
        if mode == G.MODE_STATIC:
            kin = [k0] * size
        elif p == 0:
            kin = [k0] + [int(k) for k in _oracle().adapt_k_sequence(us)[:-1]]
        else:
            total, kin = 0, [k0]
            for i, v in enumerate(us[:-1]):
                total += v
                kin.append(G.stateless_k(total, i + 1))
        toks, i = [], 0
        while i < size:
            v, k = us[i], kin[i]
            if mode in (G.MODE_RICE, G.MODE_STATIC):
                toks.append(("v", start + i, v, k))
            elif mode == G.MODE_BIN:
                toks.append(("z" if v == 0 else "s" if v <= 4 else "f", start + i, v, k))
            elif v == 0:
                j = i
                while j < size and us[j] == 0:
                    j += 1
                if j - i >= G.ZERO_RUN_MIN:
                    toks.append(("r", start + i, j - i, k))
                else:
                    toks += [("n", start + q, 0, kin[q]) for q in range(i, j)]
                i = j
                continue
            else:
                toks.append(("e" if v > (1 << min(k + 3, 24)) else "n", start + i, v, k))
            i += 1
        out.append((mode, k0, start, size, toks))
        start += size
    return out


def rewrite(x, record, parts):
    """The channel block written by lacgrammar from the tokens of tokens_of: equal to the oracle's bytes exactly when the
    tokens are the ones the encoder chose."""
    def tok(kind, value):
        if kind == "r":
            return ("r", value)
        return ("z",) if kind == "z" else (kind, G.unzigzag(value))

    cb = G.ChannelBlock(len(x), record.predictor_type, record.order, list(record.coef), record.partition_order,
                        [G.Part(mode, k0, tokens=[tok(t[0], t[2]) for t in toks]) for mode, k0, _, _, toks in parts])
    return G.write_channel_block(cb, long_ok=True)[0]


def run_placements(parts):
    """{(length, where)} of the zero runs of 1..5 samples in zero-run partitions that touch a chunk border: `starts` at a
    multiple of 16, `ends` just before one, `across` one."""
    out = set()
    for mode, _, start, size, toks in parts:
        if mode != G.MODE_ZERO_RUN:
            continue
        zero = sorted(q for kind, pos, val, _ in toks if kind == "r" or (kind == "n" and val == 0)
                      for q in range(pos, pos + (val if kind == "r" else 1)))
        runs, a = [], None
        for q in zero:
            if a is None or q != b + 1:
                if a is not None:
                    runs.append((a, b))
                a = q
            b = q
        if a is not None:
            runs.append((a, b))
        for a, b in runs:
            length = b - a + 1
            if length > 5 or a == start or b == start + size - 1:
                continue
            if a % CHUNK == 0:
                out.add((length, "starts"))
            if (b + 1) % CHUNK == 0:
                out.add((length, "ends"))
            if a // CHUNK != b // CHUNK:
                out.add((length, "across"))
    return out


WANT_PLACEMENTS = {(length, where) for length in range(1, 6) for where in ("starts", "ends", "across")} - {(1, "across")}


def check_tokens(exp):
    """What each block of the family `tokens` was chosen for, from its tokens; the tokens themselves are held against the
    oracle's bytes first."""
    facts = {}
    for b, rec, data in exp:
        parts = tokens_of(b.x, rec)
        assert rewrite(b.x, rec, parts) == data, b.name
        facts[b.name] = parts
    for n in TOKEN_N:
        # the escape inside zero-run partitions; run tokens of hundreds
        parts = facts[f"sparse_escapes_n{n}"]
        esc = [t for mode, _, _, _, toks in parts if mode == G.MODE_ZERO_RUN for t in toks if t[0] == "e"]
        assert len(esc) >= 10 and all(v > (1 << min(k + 3, 24)) for _, _, v, k in esc), (n, len(esc))
        # zero but for one partition; a run of >= 4096 as one token; a run that ends exactly at a partition end
        parts = facts[f"one_partition_n{n}"]
        x = block("tokens", f"one_partition_n{n}").x
        assert len(parts) >= 2 and x[:parts[0][3]].any() and not x[parts[0][3]:].any()
        assert {mode for mode, *_ in parts} == {G.MODE_ZERO_RUN}
        runs = [(pos, val, start + size) for _, _, start, size, toks in parts for kind, pos, val, _ in toks if kind == "r"]
        assert max(val for _, val, _ in runs) >= 4096, n
        first = [r for r in runs if r[0] < parts[0][3]]
        assert any(pos + val == end and pos > 0 for pos, val, end in first), n  # cut at the end of the first partition
        assert all(val == size for _, _, start, size, toks in parts[1:] for _, _, val, _ in toks)
        # runs of 1..5 zeros at, before and across chunk borders
        got = run_placements(facts[f"short_runs_n{n}"])
        assert got == WANT_PLACEMENTS, (n, sorted(WANT_PLACEMENTS - got))
        # unary parts of >= 32 and >= 64 ones in Rice and static partitions
        parts = facts[f"outliers_n{n}"]
        q = [v >> k for mode, _, _, _, toks in parts if mode in (G.MODE_RICE, G.MODE_STATIC) for _, _, v, k in toks]
        assert any(32 <= v < 64 for v in q) and any(v >= 64 for v in q), (n, max(q))
        # a bin partition with all four token shapes: zero, +-1, +-2, fallback
        shapes = [{"z" if kind == "z" else "f" if kind == "f" else ("s1" if v <= 2 else "s2") for kind, _, v, _ in toks}
                  for mode, _, _, _, toks in facts[f"bin_n{n}"] if mode == G.MODE_BIN]
        assert {"z", "s1", "s2", "f"} in shapes, (n, shapes)
    return facts


def check_coverage(exp=None):
    """Every condition the corpus is there for, on the oracle's records with both flags on."""
    exp = exp or {f: expected(f) for f in FAMILIES}
    assert sum(len(v) for v in exp.values()) == len(corpus()) <= 150
    assert {bits for _, _, bits in STEREO_PAIRS} == {16, 24}
    for rows in exp.values():
        for b, rec, data in rows:
            assert rec.payload_bytes == len(data), b.name  # inside the validated domain plan and emit agree

    # geometry: every order at every size, all modes, borders inside chunks, long last partitions
    reached, part_modes, ragged_last, inside = {}, set(), set(), set()
    for b, rec, _ in exp["geometry"]:
        n, p = b.x.size, rec.partition_order
        assert b.name == f"n{n}_p{p}", (b.name, p)
        reached.setdefault(n, set()).add(p)
        part_modes |= _modes(rec)
        assert len(rec.part_mode_k) == 1 << p
        if n % (1 << p):
            ragged_last.add(p)
        if n % (CHUNK << p):
            inside.add(p)
    assert reached == {n: set(range(1, max_partition_order(n) + 1)) for n in GEOMETRY_N}, reached
    assert {n: max_partition_order(n) for n in GEOMETRY_N} == \
        {4097: 7, 8191: 7, 8192: 8, 8223: 8, 12289: 8, 16368: 8, 16383: 8, 16384: 8}
    assert part_modes == {0, 1, 2, 3}, part_modes
    assert ragged_last == set(range(1, 9)) and inside >= {5, 6, 7, 8}, (ragged_last, inside)

    check_tokens(exp["tokens"])

    # parameters: the table holds 0..15 for static partitions (oracle/lac_oracle.c, estimate_static_k) and 0..12 as the
    # start of an adaptive one (estimate_initial_k); the parameter in force inside adaptive partitions takes every value up to KMAX
    static_k, start_k, in_force = set(), set(), set()
    for b, rec, data in exp["parameters"]:
        parts = tokens_of(b.x, rec)
        assert rewrite(b.x, rec, parts) == data, b.name
        for mode, k0, _, _, toks in parts:
            if mode == G.MODE_STATIC:
                static_k.add(k0)
            else:
                start_k.add(k0)
                in_force |= {k for _, _, _, k in toks}
    assert static_k == set(range(16)), sorted(static_k)
    assert start_k == START_K, sorted(start_k)
    assert in_force == IN_FORCE_K and static_k | in_force == set(range(KMAX + 1)), sorted(in_force)
    b, rec, _ = exp["parameters"][-1]
    assert b.name == "side_of_opposed_full_scale" and np.abs(b.x.astype(np.int64)).max() == EDGE - 1
    assert max(k for _, _, _, _, toks in tokens_of(b.x, rec) for _, _, _, k in toks) == KMAX

    # loud: the winner's residual sum on either side of kNarrowLimit, at partition order >= 3
    for b, rec, _ in exp["loud"]:
        total = sum(residual(b.x, rec))
        assert rec.partition_order >= 3, (b.name, rec.partition_order)
        assert total == NARROW_LIMIT - (0 if b.name.endswith("at_the_limit") else 1), (b.name, total - NARROW_LIMIT)
    assert {b.x.size for b, _, _ in exp["loud"]} == set(LOUD_N)

    # predictors: each winner at both sizes, saturated coefficients
    rows = {b.name: (b, rec) for b, rec, _ in exp["predictors"]}
    got = {}
    for n, seed, ptype, order in PREDICTORS:
        b, rec = rows[f"n{n}_seed{seed}_type{ptype}_order{order}"]
        assert (rec.predictor_type, rec.order) == (ptype, order), (b.name, rec.predictor_type, rec.order)
        got.setdefault(n, set()).add((ptype, order))
        if ptype == 2:
            assert classify(b.x, rec) == (order, order), b.name  # (no early stop inside the domain: see the docstring)
    for n, seed in FIR:
        b, rec = rows[f"n{n}_fir_seed{seed}"]
        assert (rec.predictor_type, rec.order) == (1, 2), (b.name, rec.predictor_type, rec.order)
        got[n].add((1, 2))
    assert got[16384] | got[4097] == WANT_PREDICTORS and got[4097] == WANT_PREDICTORS, got
    assert got[16384] == WANT_PREDICTORS - {(0, 1)}, got[16384]
    for n, seed in SATURATED:
        b, rec = next(v for k, v in rows.items() if k.startswith(f"n{n}_seed{seed}_type2"))
        assert set(rec.coef) & {-32768, 32767}, (b.name, rec.coef)

    # stereo: full-scale pairs whose side channel fills bits + 1 bits -- |S| >= 2^24 - 2 holds for the 24-bit pairs only,
    # the 16-bit pair reaches 2^16 - 1; M / S plans unlike L / R plans
    o = _oracle()
    for lname, rname, bits in STEREO_PAIRS:
        left, right = block("stereo", lname).x, block("stereo", rname).x
        assert fits(left, bits) and fits(right, bits) and not fits(left, bits - 1)
        m, s = planref.mid_side(left, right)
        assert np.abs(s.astype(np.int64)).max() == (1 << bits) - 1  # (24-bit pairs: |S| = 2^24 - 1 >= 2^24 - 2)
        orders = tuple(int(o.block_plan(c).partition_order) for c in (left, right, m, s))
        assert orders == STEREO_ORDERS[lname] and set(orders[2:]) != set(orders[:2]), (lname, orders)
    return {f: len(rows) for f, rows in exp.items()}


IN_FORCE_K = {12} | set(range(16, KMAX + 1))  # the parameters in force inside the family's adaptive partitions
START_K = {12}  # the table entries of the family's adaptive partitions
# partition orders the geometry blocks no longer reach without zero runs (their seeds were chosen with zero runs on)
FLAG_ORDERS_MISSED = {(False, 8192): {6}}
UNPARTITIONED_MODES = {True: {0, 1, 2, 3}, False: {0, 2, 3}}  # zero runs on / off


def check_flag_coverage():
    """The families geometry and tokens under the other three flag pairs: no partition without partitioning, no mode 1
    without zero runs, and the unpartitioned winners over the subset are of exactly the modes the pair allows."""
    for zr, pt in FLAGS[1:]:
        rows = expected("geometry", zr, pt) + expected("tokens", zr, pt)
        assert len(rows) == len(family("geometry")) + len(family("tokens"))
        if not zr:
            assert all(1 not in _modes(rec) for _, rec, _ in rows)
        if pt:
            reached, part_modes = {}, set()
            for b, rec, _ in expected("geometry", zr, pt):
                reached.setdefault(b.x.size, set()).add(rec.partition_order)
                part_modes |= _modes(rec)
            assert part_modes == UNPARTITIONED_MODES[zr], (zr, pt, part_modes)
            want = {n: set(range(1, max_partition_order(n) + 1)) - FLAG_ORDERS_MISSED.get((zr, n), set()) for n in GEOMETRY_N}
            assert reached == want, (zr, pt, reached)
        else:
            assert all(rec.partition_order == 0 and len(rec.part_mode_k) == 1 for _, rec, _ in rows)
            unpart = {rec.part_mode_k[0] >> 5 for _, rec, _ in rows}
            assert unpart == UNPARTITIONED_MODES[zr], (zr, pt, unpart)
