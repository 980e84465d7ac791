"""Hand-built .lac streams over the whole block grammar, with the samples they must decode to.

A pure-Python, seeded generator of channel blocks and of the containers around them, written from the format
(ref src/codec/block/decoder.cpp:64-520, src/codec/rice/rice.hpp:45-114, src/codec/lac/decoder.cpp:48-219).  It needs no
built library: the bits are written here, and the expected samples are computed here with Python integers.

  Bits, zigzag, unzigzag      MSB-first bit writer and the residual mapping
  Adapt, adapt_k, stateless_k Rice::adapt_k and the stateless prefix mean, restated with plain integer division
  Part, ChannelBlock          the description of one channel block: predictor, partition order, and per partition its
                              mode, initial k and either a residual list (the generator chooses the tokens, seeded)
                              or an explicit token list (directed and malformed cases)
  write_channel_block         description -> bytes, residuals, largest zigzag value written
  synthesize                  residuals -> samples (fixed 0-4, FIR, LPC), and where a sample leaves int32
  Block, make_stream          1 or 2 channels, stereo mode 0 / 1 / 2, 16 or 24 bit -> Stream (bytes + left / right)
  CASES, build(name)          the case table both test files use; WAVE_MIXES, SWEEP

A case states what the format's rules make of it: `status` 0 (valid: `left` / `right` are the answer) or the device
decoder's status code of the ONE rule it breaks (the text is in STATUS_TEXT), and `ref_ok`: whether the reference
decodes it.  The two differ only for `beyond_2p30_*` cases: the device refuses every zigzag value >= 2^30 (status 9).
"""
from __future__ import annotations

import functools
import random
import struct
from dataclasses import dataclass, field
from operator import mul

import lacstreams

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
MODE_RICE, MODE_ZERO_RUN, MODE_BIN, MODE_STATIC = 0, 1, 2, 3
ZERO_RUN_MIN, ZERO_RUN_K = 4, 2
MIN_PARTITION, MAX_PARTITION_ORDER, MAX_BLOCK, MIN_NON_FINAL = 32, 8, 16384, 256
# the device decoder's per-block status codes, as its error message spells them: "[decode-error] block=B <text>"
STATUS_TEXT = {1: "block header", 2: "channel header", 3: "residual", 4: "padding", 5: "sample overflow",
               6: "trailing bytes", 7: "sample outside the bit depth", 9: "residual beyond 2^30"}


class Bits:
    """MSB-first bit writer (the layout of ref src/codec/bitstream/bit_writer.cpp), for hand-made channel blocks."""

    def __init__(self):
        self.chunks, self.acc, self.nacc, self.n = [], 0, 0, 0

    def put(self, value, bits):
        assert 0 <= value < (1 << bits) or bits == 0
        self.acc = (self.acc << bits) | value
        self.nacc += bits
        self.n += bits
        if self.nacc >= 8192:  # whole bytes leave the accumulator, so a long block is not one huge integer
            rest = self.nacc & 7
            self.chunks.append((self.acc >> rest).to_bytes(self.nacc >> 3, "big"))
            self.acc &= (1 << rest) - 1
            self.nacc = rest

    def ones(self, count):
        while count > 0:
            c = min(count, 4096)
            self.put((1 << c) - 1, c)
            count -= c

    def rice(self, u, k):
        q = u >> k
        if q < 64:  # (the common case in one piece)
            self.put((((1 << q) - 1) << (k + 1)) | (u & ((1 << k) - 1)), q + 1 + k)
            return
        self.ones(q)                           # unary quotient: ones ...
        self.put(0, 1)                         # ... and their terminator
        self.put(u & ((1 << k) - 1), k)

    def bytes(self):
        pad = (-self.n) % 8
        return b"".join(self.chunks) + (self.acc << pad).to_bytes((self.nacc + pad) // 8, "big")


def zigzag(x):
    return (x << 1) ^ (x >> 63)


def unzigzag(u):
    return -((u >> 1) + 1) if (u & 1) else (u >> 1)


# ---- the adaptive Rice parameter (ref rice.hpp:45-114, block/decoder.cpp:90-96) ---------------------------------------
class Adapt:
    """Rice::AdaptState."""
    __slots__ = ("prev", "widx", "midx", "filled", "wsum", "large", "zero", "recent", "lflag", "zflag")

    def __init__(self):
        self.prev = self.widx = self.midx = self.filled = self.wsum = self.large = self.zero = 0
        self.recent, self.lflag, self.zflag = [0] * 256, [0] * 96, [0] * 96


def base_k(total, count):
    mean = (total + (count >> 1)) // count
    return 0 if mean <= 1 else min(31, (mean - 1).bit_length())


def stateless_k(total, count):
    return 0 if count == 0 else base_k(total, count)


def adapt_k(total, count, st):
    if count == 0:
        return 0
    cur = total - st.prev
    st.prev = total
    mi = st.midx
    st.large -= st.lflag[mi]
    st.zero -= st.zflag[mi]
    if st.filled < 256:
        st.filled += 1
    else:
        st.wsum -= st.recent[st.widx]
    st.recent[st.widx] = cur & 0xFFFFFFFF
    st.wsum += cur
    mean = (total + (count >> 1)) // count
    k = 0 if mean <= 1 else min(31, (mean - 1).bit_length())
    q = 0 if k >= 31 else (cur >> k) & 0xFFFFFFFF
    fl, fz = int(q > 3), int(q == 0)
    st.large += fl
    st.zero += fz
    st.lflag[mi], st.zflag[mi] = fl, fz
    bias = 0
    if st.filled > 0 and mean > 0:
        local = (st.wsum + 128) >> 8 if st.filled == 256 else (st.wsum + (st.filled >> 1)) // st.filled
        if local * 3 > mean * 4:
            bias = 1
        elif local * 4 + 3 < mean * 3:
            bias = -1
    if st.widx + 1 >= 96 or st.filled >= 96:
        window = 96 if st.filled >= 96 else st.filled
        if st.large * 4 >= window * 3:
            bias = min(bias + 1, 1)
        elif st.zero * 5 >= window * 4:
            bias = max(bias - 1, -1)
    st.midx = 0 if st.midx + 1 == 96 else st.midx + 1
    st.widx = (st.widx + 1) & 255
    return max(0, min(31, k + bias))


def adapt_k_sequence(us):
    """The parameter in force after each value of a stateful partition (what oracle.adapt_k_sequence returns)."""
    st, total, out = Adapt(), 0, []
    for i, u in enumerate(us):
        total += u
        out.append(adapt_k(total, i + 1, st))
    return out


# ---- one channel block -----------------------------------------------------------------------------------------------
@dataclass
class Part:
    """One partition: mode, the k of its table entry, and its content -- `res` (residuals; the tokens are the generator's
    seeded choice, see `style`) or `tokens` (explicit):
      ("v", r)       bare Rice code (modes 0 and 3)
      ("n", r) ("r", run) ("e", r)          zero-run mode: normal, run of `run` zeros, 32-bit escape
      ("z",) ("s", +-1 | +-2) ("f", r)      bin mode: zero, small value, fallback Rice code
      ("q", q, rem)  a Rice code given as quotient and remainder, behind the mode's tag for one
      ("raw", value, bits)                  bits as they are
    style: run = "token" | "normal" | "mixed" (zero runs of >= 4), split (run tokens shorter than the run), esc_p (any
    value as an escape), fb_p (a small value as the fallback code)."""
    mode: int
    k: int
    res: list = None
    tokens: list = None
    style: dict = field(default_factory=dict)
    seed: int = 0
    table_mode: int = None  # the mode written into the table, where it is to differ


@dataclass
class ChannelBlock:
    n: int
    ptype: int = 0          # 0 fixed, 1 FIR, 2 LPC
    order: int = 0
    coefs: list = field(default_factory=list)
    porder: int = 0
    parts: list = field(default_factory=list)
    raw: dict = field(default_factory=dict)  # overrides for malformed blocks: type, order, control, pad, cut (bytes kept)


def partition_sizes(n, p):
    if p == 0:
        return [n]
    base = n >> p
    return [base] * ((1 << p) - 1) + [n - base * ((1 << p) - 1)]


class TooLong(Exception):
    """A unary part too long to be worth writing: the description wants another mode or k."""


UNARY_CAP = 1 << 16


def _write_part(w, part, size, stateless, info):
    mode, k = part.mode, part.k
    total = count = 0
    st = None if stateless else Adapt()
    res = []

    def adapt(u):
        nonlocal total, count, k
        total += u
        count += 1
        k = stateless_k(total, count) if stateless else adapt_k(total, count, st)

    def rice(u):
        if (u >> k) > UNARY_CAP and not info.get("long_ok"):
            raise TooLong()
        w.rice(u, k)

    def emit(tok):
        nonlocal k, count
        t = tok[0]
        if t == "raw":
            w.put(tok[1], tok[2])
            return
        if t == "r":
            run = tok[1]
            w.put(1, 2)
            w.rice(run - ZERO_RUN_MIN, ZERO_RUN_K)
            res.extend([0] * run)
            if stateless:  # the count jumps by the run, the parameter is recomputed once
                count += run
                k = stateless_k(total, count)
            else:
                for _ in range(run):
                    adapt(0)
            return
        if t == "q":
            if mode == MODE_ZERO_RUN:
                w.put(0, 2)
            elif mode == MODE_BIN:
                w.put(3, 2)
            w.ones(tok[1])
            w.put(0, 1)
            w.put(tok[2], k)
            u = ((tok[1] << k) | tok[2]) & 0xFFFFFFFF
        elif t == "z":
            w.put(0, 2)
            u = 0
        elif t == "s":
            assert tok[1] in (1, -1, 2, -2)
            w.put(abs(tok[1]), 2)
            w.put(1 if tok[1] < 0 else 0, 1)
            u = zigzag(tok[1])
        else:
            u = zigzag(tok[1])
            assert 0 <= u < (1 << 32)
            if t == "e":
                w.put(2, 2)
                w.put(u, 32)
            else:
                if t == "n":
                    w.put(0, 2)
                elif t == "f":
                    w.put(3, 2)
                else:
                    assert t == "v"
                rice(u)
        res.append(unzigzag(u))
        info["max_u"] = max(info["max_u"], u)
        if mode != MODE_STATIC:
            adapt(u)

    if part.tokens is not None:
        for tok in part.tokens:
            emit(tok)
        return res
    r, sty, rng = part.res, part.style, random.Random(part.seed)
    assert len(r) == size, (len(r), size)
    run_style, esc_p, fb_p = sty.get("run", "mixed"), sty.get("esc_p", 0.0), sty.get("fb_p", 0.0)
    i = 0
    while i < size:
        v = r[i]
        if mode == MODE_STATIC:  # (emit(("v", v)), in place)
            u = zigzag(v)
            if (u >> k) > UNARY_CAP and not info.get("long_ok"):
                raise TooLong()
            w.rice(u, k)
            res.append(v)
            if u > info["max_u"]:
                info["max_u"] = u
        elif mode == MODE_RICE:
            emit(("v", v))
        elif mode == MODE_ZERO_RUN:
            if v == 0:
                j = i
                while j < size and r[j] == 0:
                    j += 1
                run = j - i
                as_token = run >= ZERO_RUN_MIN and (run_style == "token" or (run_style == "mixed" and rng.random() < 0.7))
                if as_token:
                    if sty.get("split") and rng.random() < 0.5:
                        run = rng.randint(ZERO_RUN_MIN, run)
                    emit(("r", run))
                    i += run
                    continue
                emit(("e", 0) if rng.random() < esc_p else ("n", 0))
            elif rng.random() < esc_p or (zigzag(v) >> k) > 2048:
                emit(("e", v))
            else:
                emit(("n", v))
        else:
            if abs(v) <= 2 and rng.random() >= fb_p:
                emit(("z",) if v == 0 else ("s", v))
            else:
                emit(("f", v))
        i += 1
    return res


def write_channel_block(cb: ChannelBlock, long_ok=False):
    """(bytes, residuals, largest zigzag value written)."""
    w, raw = Bits(), cb.raw
    info = {"max_u": 0, "long_ok": long_ok}
    w.put(raw.get("type", cb.ptype), 8)
    w.put(raw.get("order", cb.order), 8)
    if cb.ptype == 2:
        for c in cb.coefs:
            w.put(c & 0xFFFF, 16)
    p = cb.porder
    control = ((0x80 | p) if p else 0) | (cb.parts[0].mode << 5)
    w.put(raw.get("control", control), 8)
    for part in cb.parts:
        w.put(part.mode if part.table_mode is None else part.table_mode, 2)
        w.put(part.k, 5)
    res = []
    for part, size in zip(cb.parts, partition_sizes(cb.n, p)):
        res += _write_part(w, part, size, p > 0, info)
    pad = (-w.n) % 8
    w.put(raw.get("pad", 0) & ((1 << pad) - 1), pad)
    data = w.bytes()
    if "cut" in raw:
        data = data[:raw["cut"]]
    return data, res, info["max_u"]


def predict(ptype, order, coefs, out, i):
    """The prediction of sample i from out[:i] (ref block/decoder.cpp:308-403)."""
    if ptype == 0:
        if i < order or order == 0:
            return 0
        taps = ((), (1,), (2, -1), (3, -3, 1), (4, -6, 4, -1))[order]
        return sum(c * out[i - 1 - t] for t, c in enumerate(taps))
    if ptype == 1:
        return 0 if i < 2 else (3 * out[i - 1] - out[i - 2]) >> 2
    taps = min(order, i)  # taps that reach before the block start are left out
    if taps == 0:
        return 0
    return sum(map(mul, coefs[:taps], out[i - 1::-1] if taps == i else out[i - 1:i - 1 - taps:-1])) >> 15


def synthesize(ptype, order, coefs, res):
    """(samples, index of the first sample that leaves int32 or None)."""
    out = []
    for i, r in enumerate(res):
        s = r + predict(ptype, order, coefs, out, i)
        if not INT32_MIN <= s <= INT32_MAX:
            return out, i
        out.append(s)
    return out, None


def residuals_of(ptype, order, coefs, samples):
    """The residuals that make the predictor give back `samples`."""
    samples = list(samples)
    return [s - predict(ptype, order, coefs, samples, i) for i, s in enumerate(samples)]


# ---- streams ---------------------------------------------------------------------------------------------------------
@dataclass
class Block:
    chans: list             # one ChannelBlock per channel (mid and side where ms)
    ms: int = 0             # the per-block flag byte of stereo mode 2; modes 0 / 1 imply it
    raw: dict = field(default_factory=dict)  # flag (flag byte as written), tail (bytes appended)


@dataclass
class Stream:
    lac: bytes
    left: list
    right: list
    channels: int
    bit_depth: int
    rate: int
    stereo_mode: int
    frames: list            # per block
    max_u: int
    first_bad: tuple        # (block, status) of the first block this generator sees fail (5 / 7 only), or None
    status: int = 0         # expected: 0, or the device status of the case's one defect
    bad_block: int = 0
    ref_ok: bool = True


def frame_header(channels, stereo_mode, rate, bit_depth, version=3):
    return bytes([0x4C, 0x41, version, channels, stereo_mode, (rate >> 8) & 0xFF, rate & 0xFF, (rate >> 16) & 0xFF,
                  bit_depth, 0])


def make_stream(blocks, channels=1, bit_depth=24, rate=48000, stereo_mode=0, long_ok=False) -> Stream:
    lo, hi = -(1 << (bit_depth - 1)), (1 << (bit_depth - 1)) - 1
    ent, payload, left, right, frames = [], [], [], [], []
    max_u, first_bad = 0, None
    for b, blk in enumerate(blocks):
        assert len(blk.chans) == channels
        n = blk.chans[0].n
        assert b + 1 == len(blocks) or n >= MIN_NON_FINAL, "a non-final block has at least 256 frames"
        ms = blk.ms if stereo_mode == 2 else stereo_mode
        data = bytes([blk.raw.get("flag", ms)]) if (channels == 2 and stereo_mode == 2) else b""
        outs = []
        for cb in blk.chans:
            d, res, mu = write_channel_block(cb, long_ok)
            data += d
            max_u = max(max_u, mu)
            out, bad = synthesize(cb.ptype, cb.order, cb.coefs, res)
            if bad is not None and first_bad is None:
                first_bad = (b, 5)
            outs.append(out + [0] * (n - len(out)))
        data += blk.raw.get("tail", b"")
        if channels == 2 and ms:  # ref lac/decoder.cpp:48-65
            l = [m + ((s + (s & 1)) >> 1) for m, s in zip(*outs)]
            outs = [l, [a - s for a, s in zip(l, outs[1])]]
        if first_bad is None and any(not lo <= s <= hi for o in outs for s in o):
            first_bad = (b, 7)
        left += outs[0]
        if channels == 2:
            right += outs[1]
        ent.append((n, len(data)))
        payload.append(data)
        frames.append(n)
    lac = lacstreams._build(frame_header(channels, stereo_mode, rate, bit_depth), ent, b"".join(payload))
    return Stream(lac, left, right if channels == 2 else None, channels, bit_depth, rate, stereo_mode, frames, max_u,
                  first_bad)


def mid_side(left, right):
    """The mid / side channels whose inverse gives left / right."""
    side = [a - b for a, b in zip(left, right)]
    return [a - ((s + (s & 1)) >> 1) for a, s in zip(left, side)], side


# ---- building blocks of the case table -------------------------------------------------------------------------------
def _kfor(us):
    """A sensible Rice parameter for these magnitudes."""
    return min(31, (sum(us) // max(1, len(us))).bit_length()) if us else 0


def block_of(samples, ptype=0, order=0, coefs=(), porder=0, modes=(MODE_STATIC,), ks=None, style=None, seed=0, kbias=0):
    """A valid channel block that decodes to `samples`: modes rotate over the partitions, k from the partition's own
    magnitudes (plus kbias) unless given."""
    n = len(samples)
    coefs = list(coefs)
    res = residuals_of(ptype, order, coefs, samples)
    parts, off = [], 0
    for i, size in enumerate(partition_sizes(n, porder)):
        r = res[off:off + size]
        off += size
        mode = modes[i % len(modes)]
        us = [zigzag(v) for v in r]
        if ks is not None:
            k = ks[i % len(ks)]
        else:
            k = max(0, min(31, _kfor(us) + kbias))
            if mode in (MODE_STATIC, MODE_RICE, MODE_BIN):  # no escape: keep the longest unary part short
                k = max(k, max(us).bit_length() - 11)
        parts.append(Part(mode, k, res=r, style=dict(style or {}), seed=seed * 1009 + i))
    return ChannelBlock(n, ptype, order, coefs, porder, parts)


def noise(rng, n, amp):
    return [rng.randint(-amp, amp) for _ in range(n)]


def walk(rng, n, step, lo, hi):
    out, x = [], 0
    for _ in range(n):
        x = max(lo, min(hi, x + rng.randint(-step, step)))
        out.append(x)
    return out


def sparse(rng, n, amp, density):
    """Mostly zeros (runs of every length), values now and then."""
    out = []
    while len(out) < n:
        out += [0] * rng.choice((0, 1, 3, 4, 5, 16, 67, 68, 300))
        out += [rng.randint(-amp, amp) for _ in range(rng.randint(1, max(1, int(8 * density))))]
    return out[:n]


def rand_coefs(rng, order, scale):
    return [rng.randint(-scale, scale) for _ in range(order)]


def mono(cb_or_list, **kw):
    cbs = cb_or_list if isinstance(cb_or_list, list) else [cb_or_list]
    return make_stream([Block([cb]) for cb in cbs], **kw)


CASES = {}      # name -> builder() -> Stream with status / bad_block / ref_ok set
V2_SUBSET = []  # names whose version-2 rewrite goes through the serial kernel


def case(name, status=0, ref_ok=None, bad_block=0, v2=False):
    def deco(fn):
        def builder():
            s = fn()
            s.status, s.bad_block = status, bad_block
            s.ref_ok = (status == 0) if ref_ok is None else ref_ok
            if status == 0:
                assert s.first_bad is None and s.max_u < (1 << 30), name
            elif status in (5, 7):
                assert s.first_bad == (bad_block, status), (name, s.first_bad)
            if status == 9 or name.startswith("beyond_2p30_"):
                assert status == 9 and name.startswith("beyond_2p30_") and s.max_u >= (1 << 30), name
            else:
                assert s.max_u < (1 << 30), name
            return s
        assert name not in CASES
        CASES[name] = builder
        if v2:
            V2_SUBSET.append(name)
        return fn
    return deco


@functools.lru_cache(maxsize=None)
def build(name) -> Stream:
    return (CASES.get(name) or WAVE_MIXES.get(name) or SWEEP[name])()


def _rng(name):
    return random.Random("lacgrammar:" + name)


HI24, LO24 = (1 << 23) - 1, -(1 << 23)

# -- LPC orders 1..32 at n = order + 1, a mid length and 16384 (taps beyond twelve come from the history ring) ------------
for _o in range(1, 33):
    def _lpc(o=_o, n=None, tag=""):
        rng = _rng(f"lpc{o}{tag}")
        n = o + 1 if n is None else n
        co = rand_coefs(rng, o, rng.choice((500, 3000, 20000)))
        sm = walk(rng, n, 40000, LO24, HI24)
        p = rng.choice([q for q in range(0, 9) if q == 0 or (n >> q) >= MIN_PARTITION])
        modes = [(MODE_STATIC,), (MODE_RICE, MODE_STATIC), (MODE_ZERO_RUN, MODE_BIN, MODE_STATIC, MODE_RICE)][o % 3]
        return mono(block_of(sm, 2, o, co, p, modes, seed=o))
    case(f"lpc_o{_o}_min", v2=_o in (1, 13, 32))(functools.partial(_lpc, _o, None, "min"))
    case(f"lpc_o{_o}_mid", v2=_o in (7, 20))(functools.partial(_lpc, _o, 600 + 37 * _o, "mid"))
    case(f"lpc_o{_o}_full")(functools.partial(_lpc, _o, MAX_BLOCK, "full"))


@case("lpc_order_eq_n", status=2)
def _():
    cb = block_of(noise(_rng("oeq"), 8, 1000), 2, 8, rand_coefs(_rng("oeq"), 8, 500))
    return mono(cb)


@case("lpc_order_0", status=2)
def _():
    cb = block_of(noise(_rng("o0"), 300, 1000), 2, 0, [])
    return mono(cb)


# -- extreme coefficients, history at the bit-depth limits -------------------------------------------------------------
def _limits(n, rng):
    """Samples at +-the 24-bit limit: long stretches of each, alternation, and a noisy tail."""
    out = [HI24] * 70 + [LO24] * 70 + [HI24 if i & 1 else LO24 for i in range(70)]
    out += [rng.choice((HI24, LO24, HI24 - 1, LO24 + 1, 0)) for _ in range(n - len(out))]
    return out[:n]


for _name, _cf in (("pos", lambda i: 32767), ("neg", lambda i: -32768), ("alt", lambda i: 32767 if i & 1 else -32768),
                   ("alt2", lambda i: -32768 if i & 1 else 32767)):
    for _o in (1, 2, 11, 12, 13, 32):
        def _ext(o=_o, cf=_cf, tag=_name):
            rng = _rng(f"ext{tag}{o}")
            co = [cf(i) for i in range(o)]
            modes = (MODE_STATIC,) if o <= 12 else (MODE_ZERO_RUN, MODE_STATIC)
            return mono(block_of(_limits(700, rng), 2, o, co, 0 if o & 1 else 2, modes, style={"esc_p": 0.05}, seed=o))
        case(f"lpc_coef_{_name}_o{_o}")(_ext)


@case("overflow_fixed", status=5)
def _():
    # order 1: the samples are the running sum of the residuals; 2^28 each leaves int32 at the eighth
    r = [1 << 28] * 7 + [(1 << 28)] + [0] * 24
    return mono(ChannelBlock(32, 0, 1, [], 0, [Part(MODE_STATIC, 28, res=r)]))


@case("overflow_lpc", status=5)
def _():
    r = [(1 << 29) - 1] * 40
    return mono(ChannelBlock(40, 2, 4, [32767] * 4, 0, [Part(MODE_STATIC, 29, res=r)]))


@case("beyond_2p30_overflow_fir", status=9, ref_ok=False)
def _():
    # (3 x1 - x2) >> 2 cannot leave int32 while every |residual| < 2^29 (the samples stay below 1.125 * 2^30, by search
    # over all sign patterns), so the FIR overflow needs values the device refuses before it: the reference and the
    # oracle refuse the overflow, the device the residual
    v = [-(1 << 31), INT32_MAX, INT32_MAX] + [0] * 29
    return mono(ChannelBlock(32, 1, 2, [], 0, [Part(MODE_ZERO_RUN, 9, tokens=[("e", x) for x in v])]))


# -- fixed orders 0-4 and FIR where the warm-up is longer than the block -----------------------------------------------
for _n in (1, 2, 3, 4, 5):
    for _pt, _o in ((0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (1, 2)):
        def _short(n=_n, pt=_pt, o=_o):
            rng = _rng(f"short{n}{pt}{o}")
            return mono(block_of(noise(rng, n, 200000), pt, o, modes=(rng.choice((0, 1, 2, 3)),), seed=n))
        case(f"{'fir' if _pt else 'fixed' + str(_o)}_n{_n}", v2=(_n == 3))(_short)


# -- Rice parameters ---------------------------------------------------------------------------------------------------
def _big_side(n, order, rng, jitter=900):
    """A 24-bit mid/side stream whose side channel is LPC with every coefficient -1.0 on a history near -2^24: the
    prediction is near order * 2^24, the residual near -(order + 1) * 2^24 -- zigzag values up to 2^30 from samples
    that are all inside the bit depth (order 31: just under 2^30; order 32: beyond)."""
    side = [-(1 << 24) + 1 + rng.randint(0, jitter) for _ in range(n)]
    left = [LO24 + (s + (1 << 24) - 1) // 2 for s in side]  # left - right = side, both in range
    right = [a - s for a, s in zip(left, side)]
    return left, right


def _big_stream(n, order, mode, k, rng, porder=0):
    left, right = _big_side(n, order, rng)
    mid, side = mid_side(left, right)
    cm = block_of(mid, 0, 1, modes=(MODE_STATIC,))
    cs = block_of(side, 2, order, [-32768] * order, porder, (mode,), ks=[k])
    s = make_stream([Block([cm, cs], ms=1)], channels=2, stereo_mode=2, long_ok=True)
    assert s.left == left and s.right == right
    return s


for _k in (0, 1, 15, 24, 29):
    for _mode, _mn in ((MODE_STATIC, "static"), (MODE_RICE, "adaptive")):
        def _ricek(k=_k, mode=_mode):
            rng = _rng(f"rice{k}{mode}")
            if k == 29:   # zigzag values just under 2^30 (quotient 1 at k = 29)
                s = _big_stream(400, 31, mode, k, rng)
                assert (1 << 30) - (1 << 17) < s.max_u < (1 << 30)
                return s
            if k == 24:   # |residual| near 9 * 2^24: quotients around 17
                sm = [LO24 + rng.randint(0, 5000) for _ in range(500)]
                return mono(block_of(sm, 2, 16, [-32768] * 16, 0, (mode,), ks=[k]), long_ok=True)
            amp = {0: 1, 1: 3, 15: 1 << 17}[k]
            return mono(block_of(noise(rng, 3000, amp), 0, 0, [], rng.choice((0, 3)), (mode,), ks=[k]))
        case(f"rice_{_mn}_k{_k}", v2=_k in (0, 29))(_ricek)


def _unary_block(run, last_bit=False):
    """Static Rice at k = 0, fixed order 0: the value `run` is `run` ones and a terminator.  32 of them, single-bit zero
    codes in between so that the terminators fall on every bit offset of a 32-bit word."""
    pos = 8 + 8 + 8 + 7  # type, order, control, one table entry
    vals = []
    for off in range(32):
        while (pos + run) % 32 != off:
            vals.append(0)
            pos += 1
        vals.append(unzigzag(run))
        pos += run + 1
    if last_bit:  # one more run whose terminator is the last bit of the block
        while (pos + run + 1) % 8 != 0:
            vals.append(0)
            pos += 1
        vals.append(unzigzag(run))
    cb = ChannelBlock(len(vals), 0, 0, [], 0, [Part(MODE_STATIC, 0, res=vals)])
    data, _, _ = write_channel_block(cb, long_ok=True)
    if last_bit:
        assert (31 + sum(zigzag(v) + 1 for v in vals)) % 8 == 0 and data[-1] == 0xFE and data[-2] == 0xFF
    return cb


for _run in (31, 32, 33, 63, 64, 65, 96, 200, 5000):
    case(f"unary_{_run}", v2=_run in (64, 5000))(lambda run=_run: mono(_unary_block(run), long_ok=True))
case("unary_terminator_last_bit")(lambda: mono(_unary_block(65, last_bit=True), long_ok=True))


@case("unary_runs_in_tagged_modes")
def _():
    """The long unary form behind a tag: zero-run normal tokens and bin fallbacks at k = 0 (stateless partitions whose mean
    stays below 1, so the parameter stays 0)."""
    vals = ([0] * 199 + [unzigzag(130)]) * 2 + [0] * 112
    cb = ChannelBlock(512, 0, 0, [], 1, [Part(MODE_ZERO_RUN, 0, res=vals[:256], style={"run": "normal"}),
                                         Part(MODE_BIN, 0, res=vals[256:], style={"fb_p": 1.0})])
    return mono(cb, long_ok=True)


# -- the quotient limit max_q = 0xFFFFFFFF >> k --------------------------------------------------------------------------
# Every value with q == max_q is >= 2^31, i.e. a residual of at least 2^30 in magnitude, and no predictor reaches that
# far from a history inside the bit depth (LPC: 32 taps * 2^15 * 2^24 >> 15 = 2^29): the reference accepts the TOKEN and
# then refuses the sample ("outside PCM bit depth"), which the pinned refusal text tells apart from the refusal of the
# token itself ("block=0 channel=primary") one quotient further.  The device refuses the value (status 9) / the token (3).
for _k in range(24, 32):
    def _qlim(k=_k, over=0):
        max_q = 0xFFFFFFFF >> k
        toks = [("v", 5), ("v", -70000), ("q", max_q + over, 0)] + [("v", 1)] * 5
        return mono(ChannelBlock(8, 0, 0, [], 0, [Part(MODE_STATIC, k, tokens=toks)]))
    case(f"beyond_2p30_q_at_limit_k{_k}", status=9, ref_ok=False)(functools.partial(_qlim, _k, 0))
    case(f"q_over_limit_k{_k}", status=3)(functools.partial(_qlim, _k, 1))


# -- stateful (unpartitioned) adaptation: prefix sums beyond 2^31 and 2^32, drift, the 96-sample flag windows -----------
def _stateful_patterns():
    """name -> (zigzag magnitudes of a 16384-sample block, check(states) or None)."""
    pats = {}
    rng = _rng("stateful")
    n = MAX_BLOCK
    # ~2^19.5 on average: the prefix sum passes 2^31 near sample 2900 and 2^32 near 5800
    pats["sum_crosses_2p31_2p32"] = [rng.randint(1 << 18, (1 << 20) + (1 << 18)) for _ in range(n)]
    # exactly at the switch: the sum reaches 2^31 - 1, then 2^31, then 2^32 - 1, 2^32
    u, total = [], 0
    for limit in (1 << 31, 1 << 32):
        while total + (1 << 20) < limit - 1:
            u.append(1 << 20)
            total += 1 << 20
        u += [limit - 1 - total, 1]
        total = limit
    pats["sum_exactly_2p31_2p32"] = u + [1 << 20] * (n - len(u))
    pats["loud_then_quiet"] = [rng.randint(0, 1 << 22) for _ in range(6000)] + [rng.randint(0, 40) for _ in range(n - 6000)]
    pats["quiet_then_loud"] = [rng.randint(0, 40) for _ in range(7000)] + [rng.randint(0, 1 << 22) for _ in range(n - 7000)]
    pats["loud_quiet_alternating"] = [rng.randint(0, (1 << 21) if (i // 700) & 1 else 12) for i in range(n)]
    # 77 (76) of every 96 quotients zero: steady state, the drift window sees the same mean as the whole block
    for zeros in (77, 76):
        pats[f"zero_q_{zeros}_of_96"] = [(0 if (i % 96) < zeros else 1000 + (i % 7)) for i in range(n)]
    return pats


def _large_q_values(target):
    """`target` large quotients (q > 3 against the prefix mean) in a row inside the first 256 samples, where the drift
    window is still the whole prefix and only the micro window can bias: each value is chosen against the mean it
    itself raises.  Then quiet values."""
    us, total = [3] * 100, 300
    for _ in range(target):
        u = 16
        while (u >> base_k(total + u, len(us) + 1)) <= 3:
            u <<= 1
        us.append(u)
        total += u
    return us + [2] * (1024 - len(us))


def _stateful_case(us, mode, seed, style=None):
    res = [unzigzag(u) for u in us]
    assert max(abs(r) for r in res) <= HI24
    k0 = _kfor(us[:32])
    sty = dict(style or {"run": "mixed", "esc_p": 0.02, "fb_p": 0.1})
    return mono(ChannelBlock(len(res), 0, 0, [], 0, [Part(mode, k0, res=res, style=sty, seed=seed)]), long_ok=True)


def _flag_counts(us):
    """(largest large-quotient count, largest zero-quotient count) the micro window reaches from sample 96 on."""
    st, total, ml, mz = Adapt(), 0, 0, 0
    for i, u in enumerate(us):
        total += u
        adapt_k(total, i + 1, st)
        if i + 1 >= 96:
            ml, mz = max(ml, st.large), max(mz, st.zero)
    return ml, mz


STATEFUL_SEQUENCES = {}  # name -> zigzag magnitudes (the host test checks adapt_k_sequence on them)
for _pn, _us in _stateful_patterns().items():
    STATEFUL_SEQUENCES[_pn] = _us
    for _mode, _mn in ((MODE_RICE, "rice"), (MODE_ZERO_RUN, "zero_run"), (MODE_BIN, "bin")):
        case(f"stateful_{_mn}_{_pn}")(functools.partial(_stateful_case, _us, _mode, len(_pn)))
for _t in (72, 71):
    _us = _large_q_values(_t)
    assert _flag_counts(_us[:256])[0] == _t
    STATEFUL_SEQUENCES[f"large_q_{_t}_of_96"] = _us
    for _mode, _mn in ((MODE_RICE, "rice"), (MODE_ZERO_RUN, "zero_run"), (MODE_BIN, "bin")):
        case(f"stateful_{_mn}_large_q_{_t}_of_96")(functools.partial(_stateful_case, _us, _mode, _t))
assert _flag_counts(STATEFUL_SEQUENCES["zero_q_77_of_96"])[1] == 77 and _flag_counts(STATEFUL_SEQUENCES["zero_q_76_of_96"])[1] == 76


@case("stateful_zero_run_runs_adapt_per_zero")
def _():
    """Zero runs as run tokens in a stateful block: every zero of a run moves the windows (one per trip on the device)."""
    rng = _rng("zr_stateful")
    vals = []
    while len(vals) < MAX_BLOCK:
        vals += [rng.randint(-3000, 3000) for _ in range(rng.randint(1, 200))] + [0] * rng.choice((4, 5, 67, 68, 96, 97, 255, 256, 257, 700))
    vals = vals[:MAX_BLOCK]
    return mono(ChannelBlock(MAX_BLOCK, 0, 0, [], 0, [Part(MODE_ZERO_RUN, 8, res=vals, style={"run": "token"}, seed=1)]))


# -- zero-run grammar --------------------------------------------------------------------------------------------------
def _zr_vals(size, rng, first=True, last=True):
    """One partition: a run at the very start, runs of 4, 5, 67, 68 (the remainder wrap of k = 2), a run to the end."""
    v = [0] * 4 if first else [7]
    for run in (5, 67, 68, 4, 3, 2, 1):
        v += [rng.randint(1, 90) * rng.choice((1, -1))] * 2 + [0] * run
    v += [rng.randint(-50, 50) or 1 for _ in range(size - len(v) - 9)]
    return v + ([0] * 9 if last else [rng.randint(1, 9) for _ in range(9)])


@case("zero_run_runs_stateless", v2=True)
def _():
    rng = _rng("zr1")
    parts = [Part(MODE_ZERO_RUN, 5, res=_zr_vals(256, rng, i & 1 == 0, i & 2 == 0), style={"run": "token"}) for i in range(4)]
    return mono(ChannelBlock(1024, 0, 0, [], 2, parts))


@case("zero_run_runs_stateful")
def _():
    rng = _rng("zr2")
    return mono(ChannelBlock(700, 0, 1, [], 0, [Part(MODE_ZERO_RUN, 5, res=_zr_vals(700, rng), style={"run": "token"})]))


@case("zero_run_runs_spelled_out_and_split")
def _():
    rng = _rng("zr3")
    parts = [Part(MODE_ZERO_RUN, 3, res=_zr_vals(300, rng), style={"run": ("normal", "mixed")[i], "split": True, "esc_p": 0.2},
                  seed=i) for i in range(2)]
    return mono(ChannelBlock(600, 0, 0, [], 1, parts))


@case("zero_run_whole_partition_one_run")
def _():
    parts = [Part(MODE_ZERO_RUN, 0, tokens=[("r", 64)]), Part(MODE_ZERO_RUN, 4, tokens=[("n", 9)] * 60 + [("r", 4)]),
             Part(MODE_ZERO_RUN, 0, tokens=[("r", 4)] * 16), Part(MODE_ZERO_RUN, 2, tokens=[("r", 60), ("e", 0)] + [("n", 0)] * 3)]
    return mono(ChannelBlock(256, 0, 0, [], 2, parts))


def _zr_defect(tokens_tail, stateless):
    good = [("n", 3), ("n", -2), ("r", 6), ("n", 1)] * 3  # 27 samples
    if stateless:
        parts = [Part(MODE_ZERO_RUN, 3, tokens=good + tokens_tail), Part(MODE_ZERO_RUN, 3, tokens=[("n", 1)] * 32)]
        return mono(ChannelBlock(64, 0, 0, [], 1, parts))
    return mono(ChannelBlock(32, 0, 0, [], 0, [Part(MODE_ZERO_RUN, 3, tokens=good + tokens_tail)]))


for _st in (True, False):
    _sn = "stateless" if _st else "stateful"
    case(f"zero_run_to_exact_end_{_sn}")(functools.partial(_zr_defect, [("r", 5)], _st))
    case(f"zero_run_one_beyond_{_sn}", status=3)(functools.partial(_zr_defect, [("r", 6)], _st))
    case(f"zero_run_tag3_{_sn}", status=3)(functools.partial(_zr_defect, [("raw", 3, 2), ("n", 1), ("r", 4)], _st))


@case("zero_run_escapes")
def _():
    vals = [0, 1, -1, HI24, -HI24, LO24, 0, 0, 5, LO24, HI24] * 30
    return mono(ChannelBlock(len(vals), 0, 0, [], 0, [Part(MODE_ZERO_RUN, 6, tokens=[("e", v) for v in vals])]))


# -- bin grammar -------------------------------------------------------------------------------------------------------
@case("bin_all_tags", v2=True)
def _():
    rng = _rng("bin")
    vals = [0, 1, -1, 2, -2, 3, -3, 40] * 8
    for v in (0, 1, -1, 2, -2):
        vals += [v] * 150  # long stretches of one tag
    vals += [rng.choice((0, 0, 1, -1, 2, -2, 5, -9, 300)) for _ in range(1024 - len(vals))]
    parts = [Part(MODE_BIN, 1, res=vals[i * 256:(i + 1) * 256], style={"fb_p": (0.0, 0.3, 1.0, 0.5)[i]}, seed=i) for i in range(4)]
    return mono(ChannelBlock(1024, 0, 0, [], 2, parts))


@case("bin_stateful_small_values")
def _():
    rng = _rng("bin2")
    return mono(ChannelBlock(3000, 0, 2, [], 0, [Part(MODE_BIN, 0, res=residuals_of(0, 2, [], walk(rng, 3000, 2, -9000, 9000)),
                                                    style={"fb_p": 0.15}, seed=3)]))


# -- partition orders --------------------------------------------------------------------------------------------------
def _part_case(p, n, status=0):
    rng = _rng(f"part{p}_{n}")
    sm = noise(rng, n, 2000)
    for a in range(0, n, 97):
        sm[a:a + 20] = [0] * len(sm[a:a + 20])
    modes = [(MODE_RICE, MODE_ZERO_RUN, MODE_BIN, MODE_STATIC)[(i + p) & 3] for i in range(4)]
    # (status 2: n >> p is one below the smallest partition; the block is well-formed otherwise)
    return mono(block_of(sm, 0, 1, [], p, modes, style={"esc_p": 0.03, "fb_p": 0.1}, seed=p))


for _p in range(1, 9):
    case(f"partition_p{_p}_smallest_n", v2=_p in (1, 8))(functools.partial(_part_case, _p, MIN_PARTITION << _p))
    case(f"partition_p{_p}_one_below", status=2)(functools.partial(_part_case, _p, (MIN_PARTITION << _p) - 1, 2))
    case(f"partition_p{_p}_full")(functools.partial(_part_case, _p, MAX_BLOCK))
    case(f"partition_p{_p}_odd_n")(functools.partial(_part_case, _p, (40 << _p) + (1 << _p) - 1))


@case("partition_first_mode_differs_from_control", status=2)
def _():
    cb = block_of(noise(_rng("pm"), 256, 100), 0, 0, [], 2, (MODE_STATIC,))
    cb.raw["control"] = 0x80 | 2 | (MODE_RICE << 5)
    return mono(cb)


# -- header refusals: one rule each ------------------------------------------------------------------------------------
def _hdr(raw=None, ptype=0, order=0, coefs=(), porder=0, n=300, **kw):
    cb = block_of(noise(_rng("hdr"), n, 500), ptype, order, list(coefs), porder, (MODE_STATIC,))
    cb.raw.update(raw or {})
    return mono(cb, **kw)


case("header_type_3", status=2)(lambda: _hdr({"type": 3}))
case("header_fixed_order_5", status=2)(lambda: _hdr({"order": 5}))
case("header_fir_order_3", status=2)(lambda: _hdr({"order": 3}, ptype=1, order=2))
case("header_fir_order_2_is_fine")(lambda: _hdr(ptype=1, order=2))
case("header_reserved_control_bit", status=2)(lambda: _hdr({"control": (MODE_STATIC << 5) | 0x10}))
case("header_flag_without_order", status=2)(lambda: _hdr({"control": (MODE_STATIC << 5) | 0x80}))
case("header_order_without_flag", status=2)(lambda: _hdr({"control": (MODE_STATIC << 5) | 2}, porder=2))
case("header_partition_order_9", status=2)(lambda: _hdr({"control": (MODE_STATIC << 5) | 0x80 | 9}, porder=8, n=MAX_BLOCK))


@case("padding_bit_set", status=4)
def _():
    cb = block_of([3, -4, 5] * 50, 0, 0, [], 0, (MODE_STATIC,), ks=[3])
    assert (8 * 3 + 7 + 150 * 4) % 8 == 7  # one bit of padding
    cb.raw["pad"] = 1
    return mono(cb)


@case("trailing_byte", status=6)
def _():
    s = make_stream([Block([block_of(noise(_rng("tb"), 300, 500))], raw={"tail": b"\0"})])
    return s


@case("stereo_flag_byte_2", status=1)
def _():
    rng = _rng("sf")
    blk = Block([block_of(noise(rng, 300, 500)), block_of(noise(rng, 300, 500))], raw={"flag": 2})
    return make_stream([blk], channels=2, stereo_mode=2)


@case("coefficient_list_beyond_block", status=2)
def _():
    # the block ends behind an LPC header that announces 32 coefficients: refused before the list is read
    cb = block_of(noise(_rng("cl"), 300, 500), 2, 32, rand_coefs(_rng("cl"), 32, 300))
    cb.raw["cut"] = 2 + 40
    return mono(cb)


@case("partition_table_beyond_block", status=2)
def _():
    cb = block_of(noise(_rng("pt"), MAX_BLOCK, 500), 0, 0, [], 8)
    cb.raw["cut"] = 3 + 100  # the 256-entry table takes 224 bytes
    return mono(cb)


# -- stereo ------------------------------------------------------------------------------------------------------------
def _ms_stream(left, right, bit_depth, stereo_mode=2, ms=1, **kw):
    if ms:
        a, b = mid_side(left, right)
    else:
        a, b = left, right
    blk = Block([block_of(a, 0, 1, [], 0, (MODE_STATIC,)), block_of(b, 0, 0, [], 0, (MODE_ZERO_RUN,), style={"esc_p": 0.1})], ms=ms)
    s = make_stream([blk], channels=2, bit_depth=bit_depth, stereo_mode=stereo_mode, **kw)
    if s.first_bad is None:
        assert s.left == list(left) and s.right == list(right)
    return s


@case("stereo_side_parities", v2=True)
def _():
    rng = _rng("par")
    left = [rng.randint(-3000, 3000) for _ in range(800)]
    right = [a - d for a, d in zip(left, [(-5, -4, -1, 0, 1, 4, 5, 2, -2, 3, -3)[i % 11] for i in range(800)])]
    return _ms_stream(left, right, 16)


for _bd in (16, 24):
    @case(f"stereo_side_of_{_bd + 1}_bits")
    def _(bd=_bd):
        hi, lo = (1 << (bd - 1)) - 1, -(1 << (bd - 1))
        left = [hi, lo, hi, hi - 1, lo, lo + 1, 0] * 40
        right = [lo, hi, lo + 1, lo, hi - 1, hi, 0] * 40
        return _ms_stream(left, right, bd)
    for _sm in (0, 1):
        @case(f"stereo_mode_{_sm}_{_bd}bit", v2=True)
        def _(bd=_bd, sm=_sm):
            rng = _rng(f"sm{sm}{bd}")
            amp = (1 << (bd - 1)) - 1
            return _ms_stream(noise(rng, 500, amp), noise(rng, 500, amp), bd, stereo_mode=sm, ms=sm)

    @case(f"depth_one_outside_mono_{_bd}bit", status=7)
    def _(bd=_bd):
        sm = noise(_rng("d1"), 400, 1000)
        sm[377] = 1 << (bd - 1)
        return mono(block_of(sm), bit_depth=bd)

    @case(f"depth_one_outside_mid_side_{_bd}bit", status=7)
    def _(bd=_bd):
        rng = _rng("d2")
        left, right = noise(rng, 400, 1000), noise(rng, 400, 1000)
        right[13] = -(1 << (bd - 1)) - 1
        return _ms_stream(left, right, bd)


@case("beyond_2p30_valid_for_the_reference", status=9, ref_ok=True)
def _():
    s = _big_stream(300, 32, MODE_STATIC, 29, _rng("b2p30"))
    assert s.max_u >= (1 << 30) and s.first_bad is None
    return s


@case("beyond_2p30_escape", status=9, ref_ok=False)
def _():
    vals = [5, -6, 1 << 29, 7] + [0] * 28  # zigzag(2^29) = 2^30: the sample is outside the bit depth for the reference
    return mono(ChannelBlock(32, 0, 0, [], 0, [Part(MODE_ZERO_RUN, 4, tokens=[("e", v) for v in vals])]))


# ---- seeded random sweep: valid by construction, every magnitude below 2^30 ---------------------------------------------
def random_channel_block(rng, n, bit_depth, side=False, family=None):
    hi = (1 << (bit_depth - (0 if side else 1))) - 1
    lo = -hi - 1
    fam = family or rng.choice(("static", "stateless", "stateful_zr", "bin", "lpc_high", "any", "any"))
    ptype = rng.choice((0, 0, 1, 2, 2))
    if fam == "lpc_high":
        ptype = 2
    order = {0: rng.randint(0, 4), 1: 2}.get(ptype, rng.randint(13, 32) if fam == "lpc_high" else rng.randint(1, 32))
    if ptype == 2 and order >= n:
        order = n - 1
        if order == 0:
            ptype = 0
    coefs = rand_coefs(rng, order, rng.choice((200, 2000, 9000, 32767))) if ptype == 2 else []
    if ptype == 2 and fam in ("static", "stateless"):
        order = min(order, 12)
        coefs = coefs[:order]
    kind = rng.choice(("noise", "walk", "sparse", "quiet"))
    amp = 1 << rng.randint(0, bit_depth - 2)
    if kind == "noise":
        sm = noise(rng, n, amp)
    elif kind == "walk":
        sm = walk(rng, n, max(1, amp >> 4), lo, hi)
    elif kind == "sparse":
        sm = sparse(rng, n, amp, rng.random())
    else:
        sm = noise(rng, n, rng.choice((0, 1, 2, 5)))
    valid_p = [q for q in range(1, 9) if (n >> q) >= MIN_PARTITION]
    if fam == "static":
        porder, modes = rng.choice([0] + valid_p), (MODE_STATIC,)
    elif fam == "stateless":
        porder, modes = (rng.choice(valid_p) if valid_p else 0), ((MODE_RICE,) if valid_p else (MODE_STATIC,))
    elif fam == "stateful_zr":
        porder, modes = 0, (MODE_ZERO_RUN,)
    elif fam == "bin":
        porder, modes = rng.choice([0] + valid_p), (MODE_BIN,)
    else:
        porder = rng.choice([0] + valid_p)
        modes = tuple(rng.randint(0, 3) for _ in range(rng.randint(1, 5)))
    style = {"run": rng.choice(("token", "normal", "mixed")), "split": rng.random() < 0.3, "esc_p": rng.choice((0, 0.02, 0.3)),
             "fb_p": rng.choice((0, 0.1, 0.6))}
    seed = rng.randint(0, 1 << 30)
    try:
        cb = block_of(sm, ptype, order, coefs, porder, modes, style=style, seed=seed, kbias=rng.randint(-2, 2))
        write_channel_block(cb)
    except TooLong:  # a spike behind a quiet stretch in a mode without escape: the same samples in zero-run mode
        cb = block_of(sm, ptype, order, coefs, porder, (MODE_ZERO_RUN,), style=style, seed=seed)
    return cb


def random_stream(name, nblocks, sizes=None, families=None):
    rng = _rng(name)
    channels, bit_depth = rng.choice((1, 2)), rng.choice((16, 24))
    stereo_mode = rng.choice((0, 1, 2)) if channels == 2 else 0
    blocks = []
    for b in range(nblocks):
        n = sizes[b] if sizes else rng.choice((256, 257, 300, 511, 777, 1024, 1500, 2048, 4096, 4097))
        if b + 1 == nblocks and not sizes:
            n = rng.choice((1, 2, 7, 31, 33, 100, 255, 1000, 5000))
        fam = families[b % len(families)] if families else None
        ms = rng.randint(0, 1) if stereo_mode == 2 else stereo_mode
        # mid / side are drawn one bit narrower than the depth, so that left / right stay inside it
        chans = [random_channel_block(rng, n, bit_depth - (1 if ms else 0), side=bool(ms and c == 1), family=fam)
                 for c in range(channels)]
        blocks.append(Block(chans, ms=ms))
    s = make_stream(blocks, channels, bit_depth, rng.choice((44100, 48000, 96000, 192000)), stereo_mode)
    assert s.first_bad is None and s.max_u < (1 << 30), name
    return s


SWEEP = {f"sweep_{i:02d}": functools.partial(random_stream, f"sweep_{i:02d}", 14) for i in range(24)}
SWEEP["sweep_full_blocks"] = functools.partial(random_stream, "sweep_full_blocks", 6, sizes=[MAX_BLOCK] * 5 + [9999])

# ---- wave mixes: >= 64 blocks of 256..1024 frames, neighbours from different families ------------------------------------
FAMILIES = ("static", "stateless", "stateful_zr", "bin", "lpc_high")


def _mix_sizes(rng, nblocks):
    return [rng.choice((256, 300, 512, 640, 1024)) for _ in range(nblocks)]


def _plain_with_one(lane):
    name = f"wave_plain_with_one_nonplain_at_{lane}"
    fams = ["static"] * 64
    fams[lane] = "stateful_zr" if lane != 31 else "lpc_high"
    return random_stream(name, 64, sizes=_mix_sizes(_rng(name + "sz"), 64), families=fams)


WAVE_MIXES = {
    "wave_mix_rotating_families": lambda: random_stream("wave_mix_rotating_families", 80,
                                                        sizes=_mix_sizes(_rng("wm1"), 80), families=FAMILIES),
    "wave_mix_shuffled_families": lambda: random_stream(
        "wave_mix_shuffled_families", 130, sizes=_mix_sizes(_rng("wm2"), 130),
        families=[_rng("wm2f" + str(i)).choice(FAMILIES) for i in range(130)]),
    "wave_all_plain": lambda: random_stream("wave_all_plain", 64, sizes=_mix_sizes(_rng("wm3"), 64), families=("static", "stateless")),
    **{f"wave_plain_with_one_nonplain_at_{lane}": functools.partial(_plain_with_one, lane) for lane in (0, 31, 63)},
}


def failure_mix():
    """A batch of 96 mono 24-bit single-block streams that share waves: valid blocks of every family with refused cases
    in between.  [(name or None, Stream)]: each refused one must fail alone."""
    rng = _rng("failure_mix")
    refused = [n for n in CASES if build(n).status and build(n).channels == 1 and build(n).bit_depth == 24]
    out = []
    for i in range(96):
        if i % 5 == 2:
            name = refused[(i // 5) % len(refused)]
            out.append((name, build(name)))
        else:
            cb = random_channel_block(rng, rng.choice((256, 400, 1024)), 24, family=FAMILIES[i % 5])
            out.append((None, mono(cb)))
    return out


ALL_NAMES = list(CASES) + list(WAVE_MIXES) + list(SWEEP)
